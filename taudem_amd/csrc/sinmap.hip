// SinmapSI (src/SinmapSI.cpp: sindexcombined :138-441, sindexcell :449-551 and its helpers fs, f2s, f3s, fai, fai2..fai5, fa): the SINMAP stability
// index and the saturation raster.  Every cell is a function of its own inputs, so the raster is one flat array of cells here: rows play no part, a
// strip is the sub-range of its owned rows.
//
//   sinmap_classify_kernel   the first pass, streaming: a lane takes four consecutive cells - 16-byte loads of slp, sca, scamin, scamax, an 8-byte load of
//                            cal, 16-byte stores of si and sat - and evaluates each in double, in the reference's operation order (the library is built
//                            with -ffp-contract=off, so no a*b+c is fused), up to the probability integrals.  A cell that ends before them (nodata,
//                            s == 0, unstable, stable) is final; the index of every other cell goes to a list, for which a block reserves its part with
//                            one atomic (ballots per wave and cell slot, the four wave totals in LDS).  An array whose first cell is not 16-byte (cal:
//                            8-byte) aligned - a crop at an odd offset inside a larger allocation - and the last, partial group of four take element
//                            loads in the same kernel; which it is is uniform per array and per launch.
//   sinmap_heavy_kernel      the second pass: full waves of region-1/2/3 cells from the list, one cell per lane, from its inputs again; writes si.
//   sinmap_kernel            the A/B variant (TDX_SINMAP_ONEPASS=1, for scripts/bench_sinmap.py only): everything in the streaming pass, the four cells of
//                            a lane one after the other.  2.4 x slower at 16384^2 (docs/experiments_sinmap.md): a wave runs the integrals when any of its
//                            lanes needs them, and the code of four inlined copies is large.
//
// The region of a cell comes from a 65536-entry table indexed by the cal value (built on the host: first match wins, the cal nodata value and ids that
// are not listed give -1); the region's constants - tan of the friction angles, rhow / rhos - are computed on the host with the host libm
// (sinmap_table.cpp) and read from a table of 8 doubles per region.
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "context.hpp"
#include "device_common.hpp"
#include "sinmap_table.hpp"
#include "strips.hpp"

namespace {

struct SmParams {
    const double* reg;      // sinmap::REG_STRIDE doubles per region
    const int16_t* lut;     // sinmap::LUT_SIZE entries
    double rmin, rmax;      // Rminter, Rmaxter
    float slp_nodata;
};

__device__ __forceinline__ double sm_min(double a, double b) { return b < a ? b : a; }   // std::min / std::max as the reference calls them
__device__ __forceinline__ double sm_max(double a, double b) { return a < b ? b : a; }

// f2s :714-732: the distribution of the sum of two uniform variables at z
__device__ double sm_f2s(double x1, double x2, double y1, double y2, double z) {
    double p = 0.0;
    const double mn = sm_min(x1 + y2, x2 + y1), mx = sm_max(x1 + y2, x2 + y1);
    const double d1 = sm_min(x2 - x1, y2 - y1), d = z - y1 - x1, d2 = sm_max(x2 - x1, y2 - y1);
    if (z > (x1 + y1) && z < mn) p = (d * d) / (2 * (x2 - x1) * (y2 - y1));
    if (mn <= z && z <= mx) p = (d - d1 / 2) / d2;
    if (mx < z && z < (x2 + y2)) { const double e = z - y2 - x2; p = 1 - (e * e) / (2 * (x2 - x1) * (y2 - y1)); }
    if (z >= (x2 + y2)) p = 1;
    return p;
}

// fai2, fai3, fai4 :686-707 (fai5 is the identity)
__device__ __forceinline__ double sm_fai2(double y1, double y2, double b1, double b2, double a) {
    const double adiv = (y2 - y1) * (b2 - b1);
    return (a * a * log(a / (y1 * b1)) / 2 - 3 * a * a / 4 + y1 * b1 * a) / adiv;
}
__device__ __forceinline__ double sm_fai3(double y1, double y2, double b1, double b2, double a) {
    const double adiv = (y2 - y1) * (b2 - b1);
    return (a * a * log(b2 / b1) / 2 - (b2 - b1) * y1 * a) / adiv;
}
__device__ __forceinline__ double sm_fai4(double y1, double y2, double b1, double b2, double a) {
    const double adiv = (y2 - y1) * (b2 - b1);
    return (a * a * log(b2 * y2 / a) / 2 + 3 * a * a / 4 + b1 * y1 * a - b1 * y2 * a - b2 * y1 * a) / adiv;
}

// fai and fa take the pair with the smaller cross product first: y and b trade places when y1 * b2 > y2 * b1
__device__ __forceinline__ void sm_order_pairs(double& y1, double& y2, double& b1, double& b2) {
    const bool trade = y1 * b2 > y2 * b1;
    const double ya = trade ? b1 : y1, yb = trade ? b2 : y2, ba = trade ? y1 : b1, bb = trade ? y2 : b2;
    y1 = ya; y2 = yb; b1 = ba; b2 = bb;
}

// fai :639-684
__device__ double sm_fai(double y1, double y2, double b1, double b2, double a) {
    double p = 0.0;
    sm_order_pairs(y1, y2, b1, b2);
    const double a1 = y1 * b1, a2 = y1 * b2, a3 = y2 * b1, a4 = y2 * b2;
    const double c2 = -sm_fai2(y1, y2, b1, b2, a1);
    double c3, c4;
    if (a2 == 0) c3 = 0;
    else c3 = sm_fai2(y1, y2, b1, b2, a2) + c2 - sm_fai3(y1, y2, b1, b2, a2);
    if (a3 == 0) c4 = 0;
    else c4 = sm_fai3(y1, y2, b1, b2, a3) + c3 - sm_fai4(y1, y2, b1, b2, a3);
    const double c5 = sm_fai4(y1, y2, b1, b2, a4) + c4 - a4;
    if (a1 < a && a <= a2) p = sm_fai2(y1, y2, b1, b2, a) + c2;
    if (a2 < a && a <= a3) p = sm_fai3(y1, y2, b1, b2, a) + c3;
    if (a3 < a && a < a4) p = sm_fai4(y1, y2, b1, b2, a) + c4;
    if (a >= a4) p = a + c5;
    return p;
}

// fa :735-763
__device__ double sm_fa(double y1, double y2, double b1, double b2, double a) {
    double p = 0.0;
    sm_order_pairs(y1, y2, b1, b2);
    const double adiv = (y2 - y1) * (b2 - b1);
    if (y1 * b1 < a && a <= y1 * b2) p = (a * log(a / (y1 * b1)) - a + y1 * b1) / adiv;
    if (y1 * b2 < a && a <= y2 * b1) p = (a * log(b2 / b1) - (b2 - b1) * y1) / adiv;
    if (y2 * b1 < a && a < y2 * b2) p = (a * log((b2 * y2) / a) + a + b1 * y1 - b1 * y2 - b2 * y1) / adiv;
    if (a >= (b2 * y2)) p = 1;
    return p;
}

// f3s :597-636
__device__ double sm_f3s(double x1, double x2, double y1, double y2, double b1, double b2, double z) {
    if (x2 < x1 || y2 < y1 || b2 < b1) return 1000.0;
    if (x1 < 0 || y1 < 0 || b1 < 0) return 1000.0;
    if (y1 == y2 || b1 == b2) return sm_f2s(x1, x2, y1 * b1, y2 * b2, z);
    if (x2 == x1) return sm_fa(y1, y2, b1, b2, z - x1);
    return (sm_fai(y1, y2, b1, b2, z - x1) - sm_fai(y1, y2, b1, b2, z - x2)) / (x2 - x1);
}

// The state of a cell that has reached the probability integrals (the innermost else of sindexcell :517-542)
struct SmHeavy {
    double cs, ss, x1, x2, w1, w2, c1, c2, t1, t2, r;
};

__device__ double sm_regions(const SmHeavy& h) {
    const double cs = h.cs, ss = h.ss, r = h.r;
    if (h.w1 == 1) return 1 - sm_f2s(h.c1 / ss, h.c2 / ss, cs * (1 - r) / ss * h.t1, cs * (1 - r) / ss * h.t2, 1);
    const double as = 1.0 / ss;   // a / ss with a = 1
    if (h.w2 == 1) {
        const double y1 = cs / ss * (1 - r), y2 = cs / ss * (1 - h.x1 * as * r);
        const double cdf1 = (h.x2 * as - 1) / (h.x2 * as - h.x1 * as) * sm_f2s(h.c1 / ss, h.c2 / ss, cs * (1 - r) / ss * h.t1, cs * (1 - r) / ss * h.t2, 1);
        const double cdf2 = (1 - h.x1 * as) / (h.x2 * as - h.x1 * as) * sm_f3s(h.c1 / ss, h.c2 / ss, y1, y2, h.t1, h.t2, 1);
        return 1 - cdf1 - cdf2;
    }
    const double y1 = cs / ss * (1 - h.x2 * as * r), y2 = cs / ss * (1 - h.x1 * as * r);
    return 1 - sm_f3s(h.c1 / ss, h.c2 / ss, y1, y2, h.t1, h.t2, 1);
}

// One cell up to the integrals.  Returns true when the cell needs them (h is filled, sat is final, si is not); false: si and sat are final.
__device__ __forceinline__ bool sm_front(float slp, float sca, float smin, float smax, int16_t cal, const SmParams& P, float& si, float& sat, SmHeavy& h) {
    si = -1.0f;
    sat = -1.0f;
    const int ri = P.lut[uint16_t(cal)];
    if (ri < 0 || sca < 0.0f || smin < 0.0f || smax < 0.0f || slp == P.slp_nodata) return false;
    if (!(P.rmax != 0.0 || smax != 0.0f)) return false;   // the reference writes nothing: the cell keeps the partition's initial -1
    const double* R = P.reg + size_t(ri) * sinmap::REG_STRIDE;
    double x2 = (double(sca) * P.rmax + double(smax)) / R[0];
    double x1 = (double(sca) * P.rmin + double(smin)) / R[1];
    double s = double(slp);
    if (s == 0.0) { si = 10.0f; sat = 3.0f; return false; }
    s = atan(s);
    const double cs = cos(s), ss = sin(s);
    if (x1 > x2) { const double t = x2; x2 = x1; x1 = t; }
    double w2 = x2 / ss, w1 = x1 / ss;   // x * a / ss with a = 1
    double cellsat = w2;
    if (w2 > 1.0) { w2 = 1.0; cellsat = 2.0; }
    if (w1 > 1.0) { w1 = 1.0; cellsat = 3.0; }
    sat = float(cellsat);
    const double c1 = R[2], c2 = R[3], t1 = R[4], t2 = R[5], r = R[6];
    const double fs2 = (c2 + cs * (1 - w1 * r) * t2) / ss;
    double v;
    if (fs2 < 1) v = 0;
    else {
        const double fs1 = (c1 + cs * (1 - w2 * r) * t1) / ss;
        if (fs1 >= 1) v = fs1;
        else {
            h.cs = cs; h.ss = ss; h.x1 = x1; h.x2 = x2; h.w1 = w1; h.w2 = w2; h.c1 = c1; h.c2 = c2; h.t1 = t1; h.t2 = t2; h.r = r;
            return true;
        }
    }
    if (v > 10.0) v = 10.0;
    si = float(v);
    return false;
}

__device__ __forceinline__ float sm_finish(const SmHeavy& h) {
    double v = sm_regions(h);
    if (v > 10.0) v = 10.0;
    return float(v);
}

// alignment bits of the launch: set = the array's first cell is aligned for the vector access
enum { SM_AL_SLP = 1, SM_AL_SCA = 2, SM_AL_MIN = 4, SM_AL_MAX = 8, SM_AL_CAL = 16, SM_AL_SI = 32, SM_AL_SAT = 64 };

struct SmQuad { float slp[4], sca[4], smin[4], smax[4]; int16_t cal[4]; };

__device__ __forceinline__ void sm_load4(const float* __restrict__ p, unsigned long long c, int m, bool vec, float (&v)[4], float absent) {
    if (!p) { v[0] = v[1] = v[2] = v[3] = absent; return; }
    if (vec && m == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p + c);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = k < m ? p[c + k] : absent;
    }
}

__device__ __forceinline__ void sm_store4(float* __restrict__ p, unsigned long long c, int m, bool vec, const float (&v)[4]) {
    if (vec && m == 4) *reinterpret_cast<float4*>(p + c) = make_float4(v[0], v[1], v[2], v[3]);
    else {
#pragma unroll
        for (int k = 0; k < 4; k++) if (k < m) p[c + k] = v[k];
    }
}

// the four cells [c, c + m) of a lane, m = 4 but for the last lane of the range
__device__ __forceinline__ void sm_load_quad(const float* __restrict__ slp, const float* __restrict__ sca, const float* __restrict__ smin, const float* __restrict__ smax,
                                             const int16_t* __restrict__ cal, unsigned long long c, int m, unsigned al, SmQuad& q) {
    sm_load4(slp, c, m, al & SM_AL_SLP, q.slp, 0.0f);
    sm_load4(sca, c, m, al & SM_AL_SCA, q.sca, 0.0f);
    sm_load4(smin, c, m, al & SM_AL_MIN, q.smin, 0.0f);   // a road raster that was not given counts as 0
    sm_load4(smax, c, m, al & SM_AL_MAX, q.smax, 0.0f);
    if ((al & SM_AL_CAL) && m == 4) {
        const short4 s = *reinterpret_cast<const short4*>(cal + c);
        q.cal[0] = s.x; q.cal[1] = s.y; q.cal[2] = s.z; q.cal[3] = s.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) q.cal[k] = k < m ? cal[c + k] : int16_t(0);
    }
}

// A/B variant: the whole cell in the streaming pass; the four cells are four copies of the code, registers hold everything
__global__ __launch_bounds__(256) void sinmap_kernel(const float* __restrict__ slp, const float* __restrict__ sca, const float* __restrict__ smin,
                                                     const float* __restrict__ smax, const int16_t* __restrict__ cal, unsigned long long n, unsigned al, SmParams P,
                                                     float* __restrict__ si, float* __restrict__ sat) {
    const unsigned long long c = ((unsigned long long)blockIdx.x * 256ull + threadIdx.x) * 4ull;
    if (c >= n) return;
    const int m = n - c < 4ull ? int(n - c) : 4;
    SmQuad q;
    sm_load_quad(slp, sca, smin, smax, cal, c, m, al, q);
    float vsi[4], vsat[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        vsi[k] = vsat[k] = -1.0f;
        if (k < m) {
            SmHeavy h;
            if (sm_front(q.slp[k], q.sca[k], q.smin[k], q.smax[k], q.cal[k], P, vsi[k], vsat[k], h)) vsi[k] = sm_finish(h);
        }
    }
    sm_store4(si, c, m, al & SM_AL_SI, vsi);
    sm_store4(sat, c, m, al & SM_AL_SAT, vsat);
}

// First pass: everything but the integrals; the cells that need them go to `list` (their index in the range), *count of them.  A block
// reserves its part of the list with one atomic: ballots give the counts per wave and cell slot, the four wave totals meet in LDS.
__global__ __launch_bounds__(256) void sinmap_classify_kernel(const float* __restrict__ slp, const float* __restrict__ sca, const float* __restrict__ smin,
                                                              const float* __restrict__ smax, const int16_t* __restrict__ cal, unsigned long long n, unsigned al,
                                                              SmParams P, float* __restrict__ si, float* __restrict__ sat, unsigned* __restrict__ list,
                                                              unsigned long long* __restrict__ count) {
    __shared__ unsigned wave_total[4];
    __shared__ unsigned long long block_base;
    const unsigned long long c = ((unsigned long long)blockIdx.x * 256ull + threadIdx.x) * 4ull;
    const bool live = c < n;
    const int m = !live ? 0 : n - c < 4ull ? int(n - c) : 4;
    SmQuad q;
    if (live) sm_load_quad(slp, sca, smin, smax, cal, c, m, al, q);
    float vsi[4], vsat[4];
    bool heavy[4];
    unsigned before[4];   // listed cells of this wave that come before the lane's cell k: earlier slots, and lower lanes of the same slot
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned total = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        vsi[k] = vsat[k] = -1.0f;
        heavy[k] = false;
        if (k < m) {
            SmHeavy h;
            heavy[k] = sm_front(q.slp[k], q.sca[k], q.smin[k], q.smax[k], q.cal[k], P, vsi[k], vsat[k], h);
        }
        const unsigned long long mask = __ballot(heavy[k]);
        before[k] = total + unsigned(__popcll(mask & ((1ull << lane) - 1ull)));
        total += unsigned(__popcll(mask));
    }
    if (lane == 0) wave_total[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned t = wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
        block_base = t ? atomicAdd(count, (unsigned long long)t) : 0ull;
    }
    __syncthreads();
    if (total) {   // uniform in the wave
        unsigned long long base = block_base;
        for (unsigned w = 0; w < wave; w++) base += wave_total[w];
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (heavy[k]) list[base + before[k]] = unsigned(c + k);
    }
    if (live) {
        sm_store4(si, c, m, al & SM_AL_SI, vsi);
        sm_store4(sat, c, m, al & SM_AL_SAT, vsat);
    }
}

// Second pass: one listed cell per lane, from its inputs again
__global__ __launch_bounds__(256) void sinmap_heavy_kernel(const float* __restrict__ slp, const float* __restrict__ sca, const float* __restrict__ smin,
                                                           const float* __restrict__ smax, const int16_t* __restrict__ cal, SmParams P, const unsigned* __restrict__ list,
                                                           const unsigned long long* __restrict__ count, float* __restrict__ si) {
    const unsigned long long cnt = *count;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < cnt; i += (unsigned long long)gridDim.x * 256ull) {
        const size_t c = list[i];
        float vsi, vsat;
        SmHeavy h;
        if (sm_front(slp[c], sca[c], smin ? smin[c] : 0.0f, smax ? smax[c] : 0.0f, cal[c], P, vsi, vsat, h)) si[c] = sm_finish(h);
    }
}

struct SmTable {
    int32_t nreg;
    const int32_t* id;
    const float *tmin, *tmax, *cmin, *cmax, *phimin, *phimax, *rhos;
    bool ok() const { return nreg >= 0 && nreg <= 32767 && (nreg == 0 || (id && tmin && tmax && cmin && cmax && phimin && phimax && rhos)); }
};

bool sm_aligned(const void* p, size_t bytes) { return (reinterpret_cast<uintptr_t>(p) % bytes) == 0; }

// One strip (or the whole raster, a strip without halo rows): the cells of the owned rows
int sinmap_impl(tdx_context* ctx, const Strip& st, const float* d_slp, const float* d_sca, const float* d_smin, const float* d_smax, const int16_t* d_cal, float slp_nodata,
                double cal_nodata, const SmTable& T, double rminter, double rmaxter, float rhow, float* d_si, float* d_sat, tdx_stats* stats) {
    TDX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const bool compact = getenv("TDX_SINMAP_ONEPASS") == nullptr;   // (the A/B hook of scripts/bench_sinmap.py, read per call)
    std::vector<double> table;
    std::vector<int16_t> lut;
    sinmap::derive(T.nreg, T.id, T.tmin, T.tmax, T.cmin, T.cmax, T.phimin, T.phimax, T.rhos, rhow, cal_nodata, table, lut);
    const size_t off = size_t(st.y0) * size_t(st.nx);
    const unsigned long long n = (unsigned long long)(st.y1 - st.y0) * (unsigned long long)st.nx;
    double* d_reg = static_cast<double*>(ctx->scratch(TDX_S_A, (table.size() + 1) * sizeof(double)));
    int16_t* d_lut = static_cast<int16_t*>(ctx->scratch(TDX_S_B, lut.size() * sizeof(int16_t)));
    if (!d_reg || !d_lut) return TDX_ERR_NOMEM;
    unsigned* d_list = nullptr;
    unsigned long long* d_count = nullptr;
    if (compact) {
        d_list = static_cast<unsigned*>(ctx->scratch(TDX_S_C, size_t(n) * sizeof(unsigned)));
        d_count = static_cast<unsigned long long*>(ctx->scratch(TDX_S_D, sizeof(unsigned long long)));
        if (!d_list || !d_count) return TDX_ERR_NOMEM;
    }
    if (!table.empty()) TDX_HIP_CHECK(ctx, hipMemcpyAsync(d_reg, table.data(), table.size() * sizeof(double), hipMemcpyHostToDevice, s));
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(d_lut, lut.data(), lut.size() * sizeof(int16_t), hipMemcpyHostToDevice, s));
    TDX_HIP_CHECK(ctx, hipStreamSynchronize(s));   // the two host vectors end with this function
    ctx->begin_call(stats);
    strip_mark(ctx, st, "sinmapsi");
    ctx->phase = "cells";
    SmParams P{d_reg, d_lut, rminter, rmaxter, slp_nodata};
    const float *slp = d_slp + off, *sca = d_sca + off, *smin = d_smin ? d_smin + off : nullptr, *smax = d_smax ? d_smax + off : nullptr;
    const int16_t* cal = d_cal + off;
    float *si = d_si + off, *sat = d_sat + off;
    const unsigned al = (sm_aligned(slp, 16) ? SM_AL_SLP : 0) | (sm_aligned(sca, 16) ? SM_AL_SCA : 0) | (sm_aligned(smin, 16) ? SM_AL_MIN : 0) |
                        (sm_aligned(smax, 16) ? SM_AL_MAX : 0) | (sm_aligned(cal, 8) ? SM_AL_CAL : 0) | (sm_aligned(si, 16) ? SM_AL_SI : 0) |
                        (sm_aligned(sat, 16) ? SM_AL_SAT : 0);
    const unsigned grid = unsigned((n + 1023ull) / 1024ull);   // n < 2^32: at most 2^22 blocks
    {
        TdxSpan sp(ctx, TDX_K_STENCIL);
        if (!compact) {
            hipLaunchKernelGGL(sinmap_kernel, dim3(grid), dim3(256), 0, s, slp, sca, smin, smax, cal, n, al, P, si, sat);
            if (stats) stats->launches[TDX_K_STENCIL]++;
        } else {
            TDX_HIP_CHECK(ctx, hipMemsetAsync(d_count, 0, sizeof(unsigned long long), s));
            hipLaunchKernelGGL(sinmap_classify_kernel, dim3(grid), dim3(256), 0, s, slp, sca, smin, smax, cal, n, al, P, si, sat, d_list, d_count);
            const unsigned hgrid = unsigned(std::min<unsigned long long>((n + 255ull) / 256ull, (unsigned long long)ctx->num_cus * 32ull));
            hipLaunchKernelGGL(sinmap_heavy_kernel, dim3(hgrid), dim3(256), 0, s, slp, sca, smin, smax, cal, P, d_list, d_count, si);
            if (stats) stats->launches[TDX_K_STENCIL] += 2;
        }
    }
    TDX_HIP_CHECK(ctx, hipGetLastError());
    ctx->end_call();
    return TDX_OK;
}

int sinmap_check(tdx_context* ctx, const void* slp, const void* sca, const void* cal, const void* si, const void* sat, int64_t nx, int64_t ny, int64_t halo,
                 const SmTable& T, const char* who) {
    if (!ctx || !slp || !sca || !cal || !si || !sat || nx <= 0 || ny <= 0 || !T.ok()) return tdx_fail(ctx, TDX_ERR_ARG, who);
    return too_big(nx, ny + halo) ? tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip") : TDX_OK;
}

}  // namespace

extern "C" int tdx_sinmapsi_dev(tdx_context* ctx, const float* d_slp, const float* d_sca, const float* d_scamin, const float* d_scamax, const int16_t* d_cal, int64_t nx,
                                int64_t ny, float slp_nodata, double cal_nodata, int32_t nreg, const int32_t* reg_id, const float* tmin, const float* tmax,
                                const float* cmin, const float* cmax, const float* phimin, const float* phimax, const float* rhos, double rminter, double rmaxter,
                                float /*g*/, float rhow, float* d_si, float* d_sat, tdx_stats* stats) {
    const SmTable T{nreg, reg_id, tmin, tmax, cmin, cmax, phimin, phimax, rhos};
    if (int rc = sinmap_check(ctx, d_slp, d_sca, d_cal, d_si, d_sat, nx, ny, 0, T, "tdx_sinmapsi_dev: bad argument")) return rc;
    return sinmap_impl(ctx, strip_single(int(nx), int(ny)), d_slp, d_sca, d_scamin, d_scamax, d_cal, slp_nodata, cal_nodata, T, rminter, rmaxter, rhow, d_si, d_sat, stats);
}

extern "C" int tdx_sinmapsi_strip(tdx_context* ctx, const tdx_comm* comm, const float* d_slp, const float* d_sca, const float* d_scamin, const float* d_scamax,
                                  const int16_t* d_cal, int64_t nx, int64_t ny_local, float slp_nodata, double cal_nodata, int32_t nreg, const int32_t* reg_id,
                                  const float* tmin, const float* tmax, const float* cmin, const float* cmax, const float* phimin, const float* phimax, const float* rhos,
                                  double rminter, double rmaxter, float /*g*/, float rhow, float* d_si, float* d_sat, tdx_stats* stats) {
    const SmTable T{nreg, reg_id, tmin, tmax, cmin, cmax, phimin, phimax, rhos};
    if (int rc = sinmap_check(ctx, d_slp, d_sca, d_cal, d_si, d_sat, nx, ny_local, 2, T, "tdx_sinmapsi_strip: bad argument")) return rc;
    return sinmap_impl(ctx, strip_from_comm(comm, int(nx), int(ny_local)), d_slp, d_sca, d_scamin, d_scamax, d_cal, slp_nodata, cal_nodata, T, rminter, rmaxter, rhow, d_si,
                       d_sat, stats);
}

extern "C" int tdx_sinmapsi(tdx_context* ctx, const float* slp, const float* sca, const float* scamin, const float* scamax, const int16_t* cal, int64_t nx, int64_t ny,
                            float slp_nodata, double cal_nodata, int32_t nreg, const int32_t* reg_id, const float* tmin, const float* tmax, const float* cmin,
                            const float* cmax, const float* phimin, const float* phimax, const float* rhos, double rminter, double rmaxter, float g, float rhow, float* si,
                            float* sat, tdx_stats* stats) {
    const SmTable T{nreg, reg_id, tmin, tmax, cmin, cmax, phimin, phimax, rhos};
    if (!ctx || !slp || !sca || !cal || !si || !sat || nx <= 0 || ny <= 0 || !T.ok()) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_sinmapsi: bad argument");
    HostCall h(ctx, nx, ny);
    const float* d_slp = h.in(TDX_S_IO0, slp);
    const float* d_sca = h.in(TDX_S_IO1, sca);
    const float* d_min = h.in(TDX_S_IO2, scamin);   // optional
    const float* d_max = h.in(TDX_S_IO3, scamax);   // optional
    const int16_t* d_cal = h.in(TDX_S_IO4, cal);
    float* d_si = h.out(TDX_S_E, si);
    float* d_sat = h.out(TDX_S_F, sat);
    if (h.error) return h.error;
    return h.finish(tdx_sinmapsi_dev(ctx, d_slp, d_sca, d_min, d_max, d_cal, nx, ny, slp_nodata, cal_nodata, nreg, reg_id, tmin, tmax, cmin, cmax, phimin, phimax, rhos,
                                     rminter, rmaxter, g, rhow, d_si, d_sat, stats));
}
