// RetLimFlow (retlimro, src/RetlimFlow.cpp:53-240) and DinfAvalanche (avalancherunoutgrd, src/DinfAvalanche.cpp:62-420) on gfx950: the
// last two D-infinity flow-algebra tools of the reference.  Both sweep AreaDinf's dependency graph FORWARD without outlets - a cell waits
// for the neighbours whose flow reaches it and releases its at most two receivers - so they run on the forward tile sweep of
// DinfConcLimAccum (d8_sweep.hpp) with the set-up of dinf_fwd.hpp.  Everything a receiver takes from a contributor travels in the
// contributor's 16-byte record, the contributor's angle included (its proportion is recomputed with the contributor's row):
//   RetLimFlow            {qrl, angle, wg, rc}              no aux array: a cell's own wg / rc are slots of its own record
//   DinfAvalanche path    {rz, zm, dm, angle}               aux = own fel
//   DinfAvalanche direct  {rz, zm, (jm << 16 | im), angle}  aux = {own fel, own (jg << 16 | ig)}; dm is recomputed on unpack
// and two free bits of the cell's info word say "fel is data" and "the cell is a source (ass > 0)".
//
// RetLimFlow, per cell whose wg and rc are data: q = sum_k p_k * qrl_k over the neighbours with p_k > 0, p a FLOAT, float product and
// float accumulator in k = 1..8 order; q = q + wg - rc; q < 0 -> 0.  The reference does not evaluate a cell whose wg or rc is nodata and
// never releases its receivers, so everything downstream of it stays nodata.  Here such a cell is evaluated to nodata and released as
// usual, and a nodata contributor makes its receiver nodata: the same set of cells ends without a value, and the sweep has no cell that
// is ready and never evaluated.  The reference's neighbour loop tests hasAccess only, not isNodata: a neighbour WITHOUT an angle whose
// nodata value has a positive prop() (possible when the nodata value lies in (-atan2(dy, dx), 2 pi)) is added with its never-written
// qrl (-FLT_MAX) although nothing waits for it.  That needs all eight neighbours' proportions, so it is its own instantiation (ALL8),
// chosen on the host only when the nodata value of the call can send anywhere.
//
// DinfAvalanche, per cell with fel data: a source (ass > 0) starts from {alpha, 0, fel, itself}; then every contributor with p > 0,
// p >= thresh (double against the float's value) and rz >= alpha offers beta = atan((zm - fel) / d) * 180 / PI with d = dm + dist[j][k]
// (path) or the straight line from the source cell (direct); the offer wins if beta >= alpha && beta > rz so far, in k order.  beta:
// the reference calls the float atan of the host libm; here atan is evaluated in DOUBLE and rounded to float once (within half a float
// ulp of the true value), then * 180.f in float and / PI in double as in the source.  A cell whose fel is nodata is not evaluated but
// releases its receivers.  -direct: xcoord[i] = (float)(x0 + i * dlon), ycoord[j] = (float)(y3 - j * dlat) are exactly rounded fp64
// expressions and are made on the device; on a geographic raster the transcendental part of tiffIO::geotoLength (src/tiffIO.cpp:434)
// depends on the row only and comes from the host libm as three doubles per global row.  The winning d of a cell is a function of the
// cell and its source alone, so dfs is recomputed from (im, jm) when the records are unpacked; a source that kept itself gives 0.
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

constexpr unsigned AINFO_SRC = 1u << 25, AINFO_FEL = 1u << 26;   // (bits 25-31 of the info word are free in d8_sweep.hpp)
constexpr double ELIPA = 6378137.000, ELIPB = 6356752.314, BOA = ELIPB / ELIPA;   // src/tiffIO.h:96-98
constexpr int64_t DIRECT_MAX = 65536;   // (im, jm) travel as 16 + 16 bits

__device__ __forceinline__ bool is_missing(float v) { return __float_as_uint(v) == 0xFF7FFFFFu; }   // -FLT_MAX exactly: "no result"

template <bool ALL8>
struct RetLimAlg {   // src/RetlimFlow.cpp:166-207; record = {qrl, angle, wg, rc}
    using Cell = float4;
    using Aux = float;   // (unused)
    static constexpr bool HAS_AUX = false, HAS_DIST = false, HAS_ROWS = true;
    static constexpr int kBulkSweeps = 6;   // (TransLimAlg's: inherited, not measured for this policy)
    static constexpr unsigned kBulkUntil = 16;
    static constexpr int kMinWaves32 = 4;
    static constexpr int kMaxRelease = 2;
    float wg_nodata, rc_nodata;
    static __device__ __forceinline__ float head(const float4& c) { return c.x; }
    // (an angle of -FLT_MAX has no positive proportion for any cell size: a cell outside the raster sends nothing under ALL8 either)
    static __host__ __device__ __forceinline__ float4 outside() { return make_float4(TDX_ANG_NODATA, TDX_ANG_NODATA, 0.f, 0.f); }
    static __device__ __forceinline__ unsigned rel_mask(unsigned inf) { return fwd_rel_mask(inf); }
    template <class L>
    __device__ __forceinline__ void eval(L& S, int c, int cl, int ly, unsigned inf, const Cell (&nb)[9]) const {
        float4 me = S.v[cl];
        float res = TDX_ANG_NODATA;
        if (!is_nodata_f(me.z, wg_nodata) && !is_nodata_f(me.w, rc_nodata)) {
            float q = 0.f;
            bool stall = false;
#pragma unroll
            for (int k = 1; k <= 8; k++) {
                const bool dep = ((inf >> (k - 1)) & 1u) != 0u;
                if (!ALL8 && !dep) continue;
                const float4 n = nb[k];
                const float p = (float)prop_dev(n.y, (k + 4) % 8, S.rows[ly + 1 + d2(k)]);   // `float p` of src/RetlimFlow.cpp:60
                if (ALL8 && !(p > 0.f)) continue;   // (a dependency has p > 0 by construction)
                if (dep && is_missing(n.x)) stall = true;   // the reference never got here: the contributor did not release this cell
                q = q + p * n.x;
            }
            q = q + me.z - me.w;
            if (q < 0.) q = 0.f;
            res = stall ? TDX_ANG_NODATA : q;
        }
        me.x = res;
        S.v[cl] = me;
    }
};

struct DirectGeo {
    double x0, y3, dlon, dlat;   // bndbox[0], bndbox[3], ang.getdlon(), ang.getdlat() of src/DinfAvalanche.cpp:165-186
    const double* rowf;          // geographic: per GLOBAL row {elipa * cos(beta), cos(beta) / cos(lat), (elipa sin(beta))^2 + (elipb cos(beta))^2}
    int geographic;
};
// the straight line from the source cell `src` to the cell `own` (both jg << 16 | ig), src/DinfAvalanche.cpp:268-287
__device__ __forceinline__ float direct_dist(const DirectGeo& G, unsigned own, unsigned src) {
    const int ig = int(own & 0xFFFFu), jg = int(own >> 16), im = int(src & 0xFFFFu), jm = int(src >> 16);
    const float dxx = (float)(G.x0 + ig * G.dlon) - (float)(G.x0 + im * G.dlon);
    const float dyy = (float)(G.y3 - jg * G.dlat) - (float)(G.y3 - jm * G.dlat);
    if (!G.geographic) return sqrtf(dxx * dxx + dyy * dyy);
    const double* f = G.rowf + size_t(jg) * 3;   // tiffIO::geotoLength(dxx, dyy, ycoord[jg], .)
    const double dlat = (double)dyy * TDX_PI / 180., dlon = (double)dxx * TDX_PI / 180.;
    const double dbeta = dlat * BOA * f[1] * f[1];
    const double ds2 = f[2] * (dbeta * dbeta);
    const double xc = f[0] * fabs(dlon), yc = sqrt(ds2);
    return (float)sqrt(xc * xc + yc * yc);
}

// beta of src/DinfAvalanche.cpp:293: atan in double, rounded to float once, * 180 in float, / PI in double.  Not inlined: the fp64 atan inside
// the eight-neighbour loop of the sweep would push the kernel past the 128 registers a 1024-thread tile has
__device__ __noinline__ float beta_deg(float zd, float d) {
    const float at = (float)atan((double)(zd / d));
    return (float)((double)(at * 180.f) / TDX_PI);
}

template <bool PATH>
struct AvalAlg {   // src/DinfAvalanche.cpp:224-305
    using Cell = float4;
    using Aux = typename std::conditional<PATH, float, float2>::type;   // own fel; direct: and own (jg << 16 | ig)
    static constexpr bool HAS_AUX = true, HAS_DIST = PATH, HAS_ROWS = true;
    static constexpr int kBulkSweeps = 6;   // (TransLimAlg's: inherited, not measured for this policy)
    static constexpr unsigned kBulkUntil = 16;
    static constexpr int kMinWaves32 = 4;
    static constexpr int kMaxRelease = 2;
    float alpha;
    double thresh;   // the float's value: `p >= thresh` promotes it
    DirectGeo G;
    static __device__ __forceinline__ float head(const float4& c) { return c.x; }
    static __host__ __device__ __forceinline__ float4 outside() { return make_float4(TDX_ANG_NODATA, TDX_ANG_NODATA, TDX_ANG_NODATA, TDX_ANG_NODATA); }
    static __device__ __forceinline__ unsigned rel_mask(unsigned inf) { return fwd_rel_mask(inf); }
    template <class L>
    __device__ __forceinline__ void eval(L& S, int c, int cl, int ly, unsigned inf, const Cell (&nb)[9]) const {
        float4 me = S.v[cl];
        float rz = TDX_ANG_NODATA, zm = TDX_ANG_NODATA, third = TDX_ANG_NODATA;   // (direct: no source; never read while rz is nodata)
        if (inf & AINFO_FEL) {
            float fel;
            unsigned own = 0u;
            if constexpr (PATH) fel = S.aux[c];
            else { const float2 a = S.aux[c]; fel = a.x; own = __float_as_uint(a.y); }
            if (inf & AINFO_SRC) { rz = alpha; zm = fel; third = PATH ? 0.f : __uint_as_float(own); }
#pragma unroll
            for (int k = 1; k <= 8; k++) {
                if (!((inf >> (k - 1)) & 1u)) continue;
                const float4 n = nb[k];
                const double p = prop_dev(n.w, (k + 4) % 8, S.rows[ly + 1 + d2(k)]);   // the contributor's row
                if (!(p > 0.0 && p >= thresh)) continue;
                if (!(n.x >= alpha)) continue;
                float d;
                if constexpr (PATH) d = n.z + S.dist[ly * 9 + k];   // dist[j][k]: the row of the evaluated cell
                else d = direct_dist(G, own, __float_as_uint(n.z));
                const float zd = n.y - fel;
                const float beta = beta_deg(zd, d);
                if (beta >= alpha && beta > rz) { rz = beta; zm = n.y; third = PATH ? d : n.z; }
            }
        }
        me.x = rz; me.y = zm; me.z = third;
        S.v[cl] = me;
    }
};
// a record is read and written by ONE instruction - 16 bytes, 16-byte aligned
static_assert(sizeof(RetLimAlg<false>::Cell) == 16 && alignof(RetLimAlg<false>::Cell) == 16, "RetLimFlow record: one 16-byte access");
static_assert(sizeof(AvalAlg<true>::Cell) == 16 && alignof(AvalAlg<true>::Cell) == 16, "DinfAvalanche record: one 16-byte access");
static_assert(sizeof(AvalAlg<false>::Aux) == 8 && alignof(AvalAlg<false>::Aux) == 8, "DinfAvalanche direct aux: one 8-byte access");

// records of the owned rows: pending where the cell participates, "no value" elsewhere (read only under ALL8: -FLT_MAX, the reference's never-written qrl)
__global__ __launch_bounds__(256) void retlim_pack_kernel(const uint32_t* __restrict__ info, const float* __restrict__ ANG, const float* __restrict__ WG,
                                                          const float* __restrict__ RC, size_t first, size_t n, float4* __restrict__ rec) {
    const size_t i = first + size_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= first + n) return;
    rec[i] = make_float4((info[i] & d8sweep::INFO_PART) ? __uint_as_float(d8sweep::PENDING_BITS) : TDX_ANG_NODATA, ANG[i], WG[i], RC[i]);
}
// pending: on or below a cycle - never queued by the reference either
__global__ __launch_bounds__(256) void retlim_unpack_kernel(const float4* __restrict__ rec, size_t first, size_t n, float* __restrict__ qrl) {
    const size_t i = first + size_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= first + n) return;
    const float r = rec[i].x;
    qrl[i] = d8sweep::pending(r) ? TDX_ANG_NODATA : r;
}

// info bits, records and aux of the owned rows.  row_global0: global row of array row 0 (may be -1: the halo row of the first strip)
template <bool PATH>
__global__ __launch_bounds__(256) void aval_pack_kernel(uint32_t* __restrict__ info, const float* __restrict__ ANG, const float* __restrict__ FEL, float fel_nodata,
                                                        const int16_t* __restrict__ ASS, int16_t ass_nodata, int nx, int64_t row_global0, size_t first, size_t n,
                                                        float4* __restrict__ rec, typename AvalAlg<PATH>::Aux* __restrict__ aux) {
    const size_t i = first + size_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= first + n) return;
    const float fel = FEL[i];
    const int16_t ass = ASS[i];
    unsigned inf = info[i];
    if (!is_nodata_f(fel, fel_nodata)) {
        inf |= AINFO_FEL;
        if (!is_nodata_s(ass, ass_nodata) && ass > 0) inf |= AINFO_SRC;
    }
    info[i] = inf;
    rec[i] = make_float4((inf & d8sweep::INFO_PART) ? __uint_as_float(d8sweep::PENDING_BITS) : TDX_ANG_NODATA, TDX_ANG_NODATA, TDX_ANG_NODATA, ANG[i]);
    if constexpr (PATH) aux[i] = fel;
    else {
        const unsigned ig = unsigned(i % size_t(nx)), jg = unsigned(int64_t(i / size_t(nx)) + row_global0);
        aux[i] = make_float2(fel, __uint_as_float((jg << 16) | ig));
    }
}
template <bool PATH>
__global__ __launch_bounds__(256) void aval_unpack_kernel(const float4* __restrict__ rec, const typename AvalAlg<PATH>::Aux* __restrict__ aux, DirectGeo G, size_t first,
                                                          size_t n, float* __restrict__ rz, float* __restrict__ dfs) {
    const size_t i = first + size_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= first + n) return;
    const float4 r = rec[i];
    const bool has = !d8sweep::pending(r.x) && !is_missing(r.x);
    rz[i] = has ? r.x : TDX_ANG_NODATA;
    if constexpr (PATH) dfs[i] = has ? r.z : TDX_ANG_NODATA;
    else dfs[i] = has ? direct_dist(G, __float_as_uint(aux[i].y), __float_as_uint(r.z)) : TDX_ANG_NODATA;
}

// prop() of src/commonLib.cpp:76-91 on the host: can a cell whose angle is `a` send anywhere in a row with these cell sizes?
bool host_sends(float a0, double dx1, double dy1) {
    const double a2 = atan2(dy1, dx1);
    const double aref[10] = {-a2, 0., a2, 0.5 * TDX_PI, TDX_PI - a2, TDX_PI, TDX_PI + a2, 1.5 * TDX_PI, 2. * TDX_PI - a2, 2. * TDX_PI};
    for (int k = 1; k <= 8; k++) {
        float a = a0;
        double p = 0.;
        if (k == 1 && a > TDX_PI) a = (float)(a - 2.0 * TDX_PI);
        if (a > aref[k - 1] && a < aref[k + 1]) p = a > aref[k] ? (aref[k + 1] - a) / (aref[k + 1] - aref[k]) : (a - aref[k - 1]) / (aref[k] - aref[k - 1]);
        if (p >= 1e-5) return true;
    }
    return false;
}

template <bool ALL8>
int retlim_run(tdx_context* ctx, const Strip& st, float wg_nodata, float rc_nodata, FwdSetup& R, tdx_stats* stats, int64_t* rounds, int64_t* outer) {
    return fwd_sweep(ctx, st, RetLimAlg<ALL8>{wg_nodata, rc_nodata}, R, nullptr, stats, rounds, outer);
}

int retlim_impl(tdx_context* ctx, const Strip& st, float* d_ang, float ang_nodata, const double* dxc, const double* dyc, const float* d_wg, float wg_nodata,
                const float* d_rc, float rc_nodata, float* d_qrl, tdx_stats* stats) {
    TDX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t first = size_t(st.y0) * size_t(st.nx), nown = size_t(st.y1 - st.y0) * size_t(st.nx);
    // a cell counts as "without angle" within TDX_MINEPS of the nodata value (linearpart::isNodata): can any such angle send?
    bool all8 = false;
    for (int j = 0; j < st.ny_arr && !all8; j++)
        all8 = host_sends(ang_nodata, dxc[j], dyc[j]) || host_sends(ang_nodata - TDX_MINEPS, dxc[j], dyc[j]) || host_sends(ang_nodata + TDX_MINEPS, dxc[j], dyc[j]);
    FwdSetup R;
    int rc = fwd_prepare(ctx, st, d_ang, ang_nodata, dxc, dyc, nullptr, nullptr, -1, R, stats, "retlimflow");   // (no outlets)
    if (rc != TDX_OK) return rc;
    hipLaunchKernelGGL(retlim_pack_kernel, dim3(tdx_blocks_for(nown, 256)), dim3(256), 0, s, R.info, R.ang_use, d_wg, d_rc, first, nown, R.rec);
    int64_t rounds = 0, outer = 1;
    rc = all8 ? retlim_run<true>(ctx, st, wg_nodata, rc_nodata, R, stats, &rounds, &outer) : retlim_run<false>(ctx, st, wg_nodata, rc_nodata, R, stats, &rounds, &outer);
    if (rc != TDX_OK) return rc;
    hipLaunchKernelGGL(retlim_unpack_kernel, dim3(tdx_blocks_for(nown, 256)), dim3(256), 0, s, R.rec, first, nown, d_qrl);
    TDX_HIP_CHECK(ctx, hipGetLastError());
    tdx_stats* stt = stats;
    ctx->end_call();
    if (stt) { stt->rounds = outer; stt->cells_evaluated = rounds; }
    return TDX_OK;
}

struct AvalArgs {
    float* d_ang; float ang_nodata;
    const double* dxc; const double* dyc;
    const float* d_fel; float fel_nodata;
    const int16_t* d_ass; int16_t ass_nodata;
    float thresh, alpha;
    const double* geo; int geographic;   // direct: {xleftedge, ytopedge, dlon, dlat} of the whole raster (null: 0, ny_total * dyc, dxc, dyc of array row 0)
    int64_t row0, ny_total;              // global row of the first owned row, rows of the whole raster
    float* d_rz; float* d_dfs;
};

template <bool PATH>
int aval_run(tdx_context* ctx, const Strip& st, const AvalArgs& a, tdx_stats* stats) {
    using Alg = AvalAlg<PATH>;
    hipStream_t s = ctx->stream;
    const int inx = st.nx, iny = st.ny_arr;
    const size_t n = size_t(inx) * size_t(iny);
    const size_t first = size_t(st.y0) * size_t(inx), nown = size_t(st.y1 - st.y0) * size_t(inx);
    DirectGeo G{0., 0., 1., 1., nullptr, 0};
    float* d_dist = nullptr;
    if constexpr (PATH) {
        // dist[j][k] = sqrt(dxc^2 d1^2 + dyc^2 d2^2) in double, stored as float (src/DinfAvalanche.cpp:131-140); d1 / d2 of src/commonLib.h
        static const int hd1[9] = {0, 1, 1, 0, -1, -1, -1, 0, 1}, hd2[9] = {0, 0, -1, -1, -1, 0, 1, 1, 1};
        std::vector<float> dist(size_t(iny) * 9, 0.f);
        for (int m = 0; m < iny; m++)
            for (int k = 1; k <= 8; k++)
                dist[size_t(m) * 9 + size_t(k)] = (float)sqrt(a.dxc[m] * a.dxc[m] * hd1[k] * hd1[k] + a.dyc[m] * a.dyc[m] * hd2[k] * hd2[k]);
        d_dist = static_cast<float*>(ctx->scratch(TDX_S_F, dist.size() * sizeof(float)));
        if (!d_dist) return TDX_ERR_NOMEM;
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(d_dist, dist.data(), dist.size() * sizeof(float), hipMemcpyHostToDevice, s));
        TDX_HIP_CHECK(ctx, hipStreamSynchronize(s));   // `dist` is a local
    } else {
        const double xleft = a.geo ? a.geo[0] : 0., dlon = a.geo ? a.geo[2] : a.dxc[0], dlat = a.geo ? a.geo[3] : a.dyc[0];
        const double ytop = a.geo ? a.geo[1] : double(a.ny_total) * dlat;
        // tiffIO::tiffIO (src/tiffIO.cpp:100-101) and bndbox of src/DinfAvalanche.cpp:170-173, in their order of operations
        const double xllcenter = xleft + dlon / 2., yllcenter = ytop - (double(a.ny_total) * dlat) - dlat / 2.;
        const double b0 = xllcenter - (dlon / 2), b1 = yllcenter - (dlat / 2);
        G.x0 = b0; G.y3 = b1 + (dlat * double(a.ny_total)); G.dlon = dlon; G.dlat = dlat; G.geographic = a.geographic ? 1 : 0;
        if (G.geographic) {   // the row-only part of tiffIO::geotoLength(., ., ycoord[jg], .) with the host libm
            std::vector<double> f(size_t(a.ny_total) * 3);
            for (int64_t j = 0; j < a.ny_total; j++) {
                const float yc = (float)(G.y3 - int(j) * dlat);
                const double lat = (double)yc * TDX_PI / 180.;
                const double beta = atan(BOA * tan(lat));
                f[size_t(j) * 3 + 0] = ELIPA * cos(beta);
                f[size_t(j) * 3 + 1] = cos(beta) / cos(lat);
                f[size_t(j) * 3 + 2] = pow(ELIPA * sin(beta), 2) + pow(ELIPB * cos(beta), 2);
            }
            double* d_f = static_cast<double*>(ctx->scratch(TDX_S_E, f.size() * 8));
            if (!d_f) return TDX_ERR_NOMEM;
            TDX_HIP_CHECK(ctx, hipMemcpyAsync(d_f, f.data(), f.size() * 8, hipMemcpyHostToDevice, s));
            TDX_HIP_CHECK(ctx, hipStreamSynchronize(s));   // `f` is a local
            G.rowf = d_f;
        }
    }
    FwdSetup R;
    int rc = fwd_prepare(ctx, st, a.d_ang, a.ang_nodata, a.dxc, a.dyc, nullptr, nullptr, -1, R, stats, "dinfavalanche");   // (no outlets)
    if (rc != TDX_OK) return rc;
    typename Alg::Aux* aux = static_cast<typename Alg::Aux*>(ctx->scratch(TDX_S_B, n * sizeof(typename Alg::Aux)));
    if (!aux) return TDX_ERR_NOMEM;
    hipLaunchKernelGGL(aval_pack_kernel<PATH>, dim3(tdx_blocks_for(nown, 256)), dim3(256), 0, s, R.info, R.ang_use, a.d_fel, a.fel_nodata, a.d_ass, a.ass_nodata, inx,
                       a.row0 - int64_t(st.y0), first, nown, R.rec, aux);
    int64_t rounds = 0, outer = 1;
    rc = fwd_sweep(ctx, st, Alg{a.alpha, (double)a.thresh, G}, R, aux, stats, &rounds, &outer, d_dist);
    if (rc != TDX_OK) return rc;
    hipLaunchKernelGGL(aval_unpack_kernel<PATH>, dim3(tdx_blocks_for(nown, 256)), dim3(256), 0, s, R.rec, aux, G, first, nown, a.d_rz, a.d_dfs);
    TDX_HIP_CHECK(ctx, hipGetLastError());
    tdx_stats* stt = stats;
    ctx->end_call();
    if (stt) { stt->rounds = outer; stt->cells_evaluated = rounds; }
    return TDX_OK;
}

int aval_impl(tdx_context* ctx, const Strip& st, const AvalArgs& a, int path, tdx_stats* stats) {
    TDX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (path) return aval_run<true>(ctx, st, a, stats);
    if (st.nx > DIRECT_MAX || a.ny_total > DIRECT_MAX)
        return tdx_fail(ctx, TDX_ERR_ARG, "dinfavalanche: -direct packs the source cell into 16 + 16 bits: rasters wider or taller than 65536 are not supported");
    if (a.geographic && !a.geo) return tdx_fail(ctx, TDX_ERR_ARG, "dinfavalanche: -direct on a geographic raster needs the geotransform");
    return aval_run<false>(ctx, st, a, stats);
}

}  // namespace

// the argument test of the _dev (halo 0) and _strip (halo 2: the strip's two halo rows) entry points
static int retlim_check(tdx_context* ctx, const void* ang, const void* wg, const void* rc_in, const void* qrl, const void* dxc, const void* dyc, int64_t nx, int64_t ny,
                        int64_t halo, const char* who) {
    if (!ctx || !ang || !wg || !rc_in || !qrl || !dxc || !dyc || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, who);
    return too_big(nx, ny + halo) ? tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip") : TDX_OK;
}

extern "C" int tdx_retlimflow_dev(tdx_context* ctx, const float* d_ang, int64_t nx, int64_t ny, float ang_nodata, const double* dxc, const double* dyc,
                                  const float* d_wg, float wg_nodata, const float* d_rc, float rc_nodata, float* d_qrl, tdx_stats* stats) {
    if (int rc = retlim_check(ctx, d_ang, d_wg, d_rc, d_qrl, dxc, dyc, nx, ny, 0, "tdx_retlimflow_dev: bad argument")) return rc;
    return retlim_impl(ctx, strip_single(int(nx), int(ny)), const_cast<float*>(d_ang), ang_nodata, dxc, dyc, d_wg, wg_nodata, d_rc, rc_nodata, d_qrl, stats);
}
extern "C" int tdx_retlimflow_strip(tdx_context* ctx, const tdx_comm* comm, float* d_ang, int64_t nx, int64_t ny_local, float ang_nodata, const double* dxc,
                                    const double* dyc, const float* d_wg, float wg_nodata, const float* d_rc, float rc_nodata, float* d_qrl, tdx_stats* stats) {
    if (int rc = retlim_check(ctx, d_ang, d_wg, d_rc, d_qrl, dxc, dyc, nx, ny_local, 2, "tdx_retlimflow_strip: bad argument")) return rc;
    return retlim_impl(ctx, strip_from_comm(comm, int(nx), int(ny_local)), d_ang, ang_nodata, dxc, dyc, d_wg, wg_nodata, d_rc, rc_nodata, d_qrl, stats);
}
extern "C" int tdx_retlimflow(tdx_context* ctx, const float* ang, int64_t nx, int64_t ny, float ang_nodata, const double* dxc, const double* dyc, const float* wg,
                              float wg_nodata, const float* rc_in, float rc_nodata, float* qrl, tdx_stats* stats) {
    if (!ctx || !ang || !wg || !rc_in || !qrl || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_retlimflow: bad argument");
    HostCall h(ctx, nx, ny);
    float* d_a = h.in(TDX_S_IO0, ang);
    float* d_w = h.in(TDX_S_IO1, wg);
    float* d_r = h.in(TDX_S_IO2, rc_in);
    float* d_o = h.out(TDX_S_IO4, qrl);
    if (h.error) return h.error;
    return h.finish(tdx_retlimflow_dev(ctx, d_a, nx, ny, ang_nodata, dxc, dyc, d_w, wg_nodata, d_r, rc_nodata, d_o, stats));
}

extern "C" int tdx_dinfavalanche_dev(tdx_context* ctx, const float* d_ang, int64_t nx, int64_t ny, float ang_nodata, const double* dxc, const double* dyc,
                                     const float* d_fel, float fel_nodata, const int16_t* d_ass, int16_t ass_nodata, float thresh, float alpha, int path,
                                     const double* geo, int geographic, float* d_rz, float* d_dfs, tdx_stats* stats) {
    if (!ctx || !d_ang || !d_fel || !d_ass || !d_rz || !d_dfs || !dxc || !dyc || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_dinfavalanche_dev: bad argument");
    if (too_big(nx, ny)) return tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip");
    const AvalArgs a{const_cast<float*>(d_ang), ang_nodata, dxc, dyc, d_fel, fel_nodata, d_ass, ass_nodata, thresh, alpha, geo, geographic, 0, ny, d_rz, d_dfs};
    return aval_impl(ctx, strip_single(int(nx), int(ny)), a, path, stats);
}
extern "C" int tdx_dinfavalanche_strip(tdx_context* ctx, const tdx_comm* comm, float* d_ang, int64_t nx, int64_t ny_local, float ang_nodata, const double* dxc,
                                       const double* dyc, const float* d_fel, float fel_nodata, const int16_t* d_ass, int16_t ass_nodata, float thresh, float alpha,
                                       int path, const double* geo, int geographic, int64_t row0, int64_t ny_total, float* d_rz, float* d_dfs, tdx_stats* stats) {
    if (!ctx || !d_ang || !d_fel || !d_ass || !d_rz || !d_dfs || !dxc || !dyc || nx <= 0 || ny_local <= 0 || row0 < 0 || ny_total < row0 + ny_local)
        return tdx_fail(ctx, TDX_ERR_ARG, "tdx_dinfavalanche_strip: bad argument");
    if (too_big(nx, ny_local + 2)) return tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip");
    const AvalArgs a{d_ang, ang_nodata, dxc, dyc, d_fel, fel_nodata, d_ass, ass_nodata, thresh, alpha, geo, geographic, row0, ny_total, d_rz, d_dfs};
    return aval_impl(ctx, strip_from_comm(comm, int(nx), int(ny_local)), a, path, stats);
}
extern "C" int tdx_dinfavalanche(tdx_context* ctx, const float* ang, int64_t nx, int64_t ny, float ang_nodata, const double* dxc, const double* dyc, const float* fel,
                                 float fel_nodata, const int16_t* ass, int16_t ass_nodata, float thresh, float alpha, int path, const double* geo, int geographic,
                                 float* rz, float* dfs, tdx_stats* stats) {
    if (!ctx || !ang || !fel || !ass || !rz || !dfs || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_dinfavalanche: bad argument");
    HostCall h(ctx, nx, ny);
    float* d_a = h.in(TDX_S_IO0, ang);
    float* d_f = h.in(TDX_S_IO1, fel);
    int16_t* d_s = h.in(TDX_S_IO2, ass);
    float* d_r = h.out(TDX_S_IO3, rz);
    float* d_d = h.out(TDX_S_IO4, dfs);
    if (h.error) return h.error;
    return h.finish(tdx_dinfavalanche_dev(ctx, d_a, nx, ny, ang_nodata, dxc, dyc, d_f, fel_nodata, d_s, ass_nodata, thresh, alpha, path, geo, geographic, d_r, d_d, stats));
}
