// The set-up of the REVERSE D8 sweeps (d8rev.hip: D8HDistToStrm, D8VDistToStrm, GageWatershed), the counterpart of dinf_rev.hpp: one streaming pass
// over the direction grid writes the info word of the dependency graph.  A cell's value comes from the ONE cell it drains to (its
// receiver); the sweep runs upstream from the sources (stream cells / gauges) and a finished cell releases the neighbours that drain
// into it.
//
// Per cell: [0:8) the receiver that counts (dependency; at most one bit), [13] INFO_PART, [16:24) neighbours that drain into the cell
// (they wait for it: the release mask).  What "drains into" means is the tool's:
//   MODE_DIST  p(n) - k == +-4 for any p(n) that is not nodata, with no sign check (src/D8HDistToStrm.cpp:189): a p == 0 neighbour counts
//              at k == 4, the quirk d8_sweep.hpp documents for AreaD8.  Stream cells (src not nodata, src >= thresh) take part whatever p
//              is, nodata included, and depend on nothing; other cells take part where p is not nodata and depend on their receiver if
//              p is 1..8 (p == 0 reads the cell's own, still unset, distance: nodata).
//   MODE_GAGE  p(n) > 0 first (src/gagewatershed.cpp:257-259).  Cells with p 1..8 take part and depend on their receiver; the gauges are
//              seeded by the caller, which clears their info word.
//   MODE_VDIST sources, participation and release of MODE_DIST (src/D8VDistToStrm.cpp:153-165, 201-219).
// MODE_DIST also writes each cell's own step into `step` (dist[j][p], float, of the cell's row j; 0 on stream cells; nodata where there
// is no receiver), so that the sweep's evaluation is one float add.  MODE_VDIST's step is the drop to the receiver, fel - fel(receiver) in
// float with no nodata test on either (src/D8VDistToStrm.cpp:191-198); a cell whose receiver lies off the array is never released, its
// step is nodata.
#pragma once
#include <vector>

#include "context.hpp"
#include "d8_sweep.hpp"
#include "device_common.hpp"

namespace d8rev {
using namespace tdxk;

enum { MODE_DIST = 0, MODE_GAGE = 1, MODE_VDIST = 2 };
constexpr int32_t GW_NODATA = -2147483647;   // MISSINGLONG (src/commonLib.h:79)

// src / step are only read / written on the owned rows [y_own0, y_own1) (the halo rows of a strip hold no src values); `dist` is [row][9]
static __global__ __launch_bounds__(256) void setup_kernel(const int16_t* __restrict__ P, int nx, int ny, int16_t nodata, int mode, const int32_t* __restrict__ src,
                                                           int32_t src_nodata, int32_t thresh, const float* __restrict__ dist, const float* __restrict__ fel, int y_own0,
                                                           int y_own1, uint32_t* __restrict__ info, float* __restrict__ step) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= nx || y >= ny) return;
    const size_t idx = size_t(y) * size_t(nx) + size_t(x);
    const int16_t p = P[idx];
    const bool pnd = is_nodata_s(p, nodata), own = y >= y_own0 && y < y_own1;
    unsigned inf = 0;
#pragma unroll
    for (int k = 1; k <= 8; k++) {
        const int xn = x + d1(k), yn = y + d2(k);
        if (xn < 0 || xn >= nx || yn < 0 || yn >= ny) continue;
        const int16_t pn = P[size_t(yn) * size_t(nx) + size_t(xn)];
        if (is_nodata_s(pn, nodata) || (mode == MODE_GAGE && pn <= 0)) continue;
        if (pn - k == 4 || pn - k == -4) inf |= 1u << (16 + k - 1);
    }
    const bool recv = !pnd && p >= 1 && p <= 8;
    if (mode != MODE_GAGE) {
        const bool stream = own && src[idx] != src_nodata && src[idx] >= thresh;   // !src->isNodata(i, j) && src >= thresh (src/D8HDistToStrm.cpp:171)
        if (stream || !pnd) inf |= d8sweep::INFO_PART;
        if (!stream && recv) inf |= 1u << (p - 1);
        if (own) {
            float stp = stream ? 0.0f : TDX_ANG_NODATA;
            if (!stream && recv) {
                if (mode == MODE_DIST) stp = dist[size_t(y) * 9 + size_t(p)];
                else {
                    const int xn = x + d1(p), yn = y + d2(p);
                    if (xn >= 0 && xn < nx && yn >= 0 && yn < ny) stp = fel[idx] - fel[size_t(yn) * size_t(nx) + size_t(xn)];
                }
            }
            step[idx] = stp;
        }
    } else if (recv) {
        inf |= d8sweep::INFO_PART | (1u << (p - 1));
    }
    info[idx] = inf;
}

// ---- what the D8 reverse policies share (d8rev.hip; streamnet.hip's label sweep is GageAlg with records of its own)
// the receiver of a cell in the lockstep form of the reverse sweep: the single dependency bit
__device__ __forceinline__ void rev_row_d8(unsigned inf, int (&k)[2], bool (&on)[2], double (&p)[2]) {
    const unsigned m = inf & 0xFFu;
    k[0] = m ? __ffs(int(m)) : 1; k[1] = k[0];
    on[0] = m != 0u; on[1] = false;
    p[0] = 0.; p[1] = 0.;
}

struct GageAlg {   // src/gagewatershed.cpp:226-233; record = index of the labelling outlet (StreamNet, src/streamnet.cpp:1397-1399: the link's id)
    using Cell = int32_t;
    using Aux = float;                              // (none)
    static constexpr bool HAS_AUX = false, HAS_DIST = false, HAS_ROWS = false;
    static constexpr int kBulkSweeps = 0;
    static constexpr unsigned kBulkUntil = 64;
    static constexpr int kMinWaves32 = 5;
    static constexpr int kMaxRelease = 8;
    static __device__ __forceinline__ float head(int32_t c) { return __int_as_float(c); }
    static __host__ __device__ __forceinline__ int32_t outside() { return GW_NODATA; }
    static __device__ __forceinline__ unsigned rel_mask(unsigned inf) { return (inf >> 16) & 0xFFu; }
    static __device__ __forceinline__ void rev_row(unsigned inf, const Aux&, double, int (&k)[2], bool (&on)[2], double (&p)[2]) { rev_row_d8(inf, k, on, p); }
    __device__ __forceinline__ Cell eval2(const Aux&, const bool (&on)[2], const double (&)[2], const Cell (&n)[2]) const { return on[0] ? n[0] : GW_NODATA; }
    template <class L>
    __device__ __forceinline__ void eval(L& S, int, int cl, int, unsigned inf, const Cell (&nb)[9]) const {
        int k[2];
        bool on[2];
        double p[2];
        rev_row_d8(inf, k, on, p);
        Cell n[2] = {GW_NODATA, GW_NODATA};
#pragma unroll
        for (int kk = 1; kk <= 8; kk++) if (kk == k[0]) n[0] = nb[kk];
        S.v[cl] = eval2(Aux{}, on, p, n);
    }
};

struct RevSetup {
    uint32_t* info = nullptr;
    uint32_t* flags = nullptr;
    unsigned long long* counts = nullptr;
};
// common front part: halo rows of the direction grid (and of MODE_VDIST's elevations), info words (and the distance modes' steps)
static int rev_prepare(tdx_context* ctx, const Strip& st, int16_t* d_p, int16_t p_nodata, int mode, const int32_t* d_src, int32_t src_nodata, int32_t thresh,
                       const double* dxc, const double* dyc, float* d_step, RevSetup& R, tdx_stats* stats, const char* stage, float* d_fel = nullptr) {
    hipStream_t s = ctx->stream;
    const int inx = st.nx, iny = st.ny_arr;
    const size_t n = size_t(inx) * size_t(iny);
    const tilek::TileGeom geom = tilek::make_geom(inx, iny, st.y0, st.y1);
    const size_t ntiles = size_t(geom.tiles_x) * size_t(geom.tiles_y);
    R.info = static_cast<uint32_t*>(ctx->scratch(TDX_S_A, n * 4));
    R.flags = static_cast<uint32_t*>(ctx->scratch(TDX_S_L, ntiles * 4 * (1 + tilek::SCHED_LIST_WORDS)));
    R.counts = static_cast<unsigned long long*>(ctx->scratch(TDX_S_M, size_t(tilek::COUNT_RING) * 16));
    if (!R.info || !R.flags || !R.counts) return TDX_ERR_NOMEM;
    float* d_dist = nullptr;
    if (mode == MODE_DIST) {
        // dist[j][k] = sqrt(d1^2 dxc^2 + d2^2 dyc^2) in double, stored as float (src/D8HDistToStrm.cpp:124-130)
        static const int hd1[9] = {0, 1, 1, 0, -1, -1, -1, 0, 1}, hd2[9] = {0, 0, -1, -1, -1, 0, 1, 1, 1};
        std::vector<float> dist(size_t(iny) * 9, 0.f);
        for (int m = 0; m < iny; m++)
            for (int k = 1; k <= 8; k++)
                dist[size_t(m) * 9 + size_t(k)] = (float)sqrt(hd1[k] * hd1[k] * dxc[m] * dxc[m] + hd2[k] * hd2[k] * dyc[m] * dyc[m]);
        d_dist = static_cast<float*>(ctx->scratch(TDX_S_F, dist.size() * sizeof(float)));
        if (!d_dist) return TDX_ERR_NOMEM;
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(d_dist, dist.data(), dist.size() * sizeof(float), hipMemcpyHostToDevice, s));
        TDX_HIP_CHECK(ctx, hipStreamSynchronize(s));   // `dist` is a local
    }
    ctx->begin_call(stats);
    strip_mark(ctx, st, stage);
    int rc = strip_exchange<int16_t>(ctx, st, d_p, p_nodata);   // p->share()
    if (rc != TDX_OK) return rc;
    if (mode == MODE_VDIST) {
        rc = strip_exchange<float>(ctx, st, d_fel, TDX_ANG_NODATA);   // fel->share(): the receiver of a boundary cell lies in the halo row
        if (rc != TDX_OK) return rc;
    }
    TdxSpan sp(ctx, TDX_K_STENCIL);
    hipLaunchKernelGGL(setup_kernel, dim3((inx + 63) / 64, (iny + 3) / 4), dim3(256), 0, s, d_p, inx, iny, p_nodata, mode, d_src, src_nodata, thresh, d_dist, d_fel,
                       st.y0, st.y1, R.info, d_step);
    if (stats) stats->launches[TDX_K_STENCIL]++;
    return TDX_OK;
}

}  // namespace d8rev
