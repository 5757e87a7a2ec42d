// The set-up shared by the REVERSE D-infinity sweeps (dinfrev.hip: DinfUpDependence, DinfRevAccum; dinfdist.hip: DinfDistDown): the info
// words of the dependency graph, the two receivers of a cell in the reference's k order, the per-row atan2 table and the halo of the
// angle grid.  A cell's value depends on its at most two downslope receivers; the sweep runs upstream from the cells without any.
#pragma once
#include <cmath>
#include <vector>

#include "context.hpp"
#include "d8_sweep.hpp"
#include "device_common.hpp"
#include "dinf_prop.hpp"

namespace dinfrev {
using namespace tdxk;

constexpr unsigned RINFO_P1 = 1u << 12, RINFO_P2 = 1u << 15;

// Per cell: [0:8) receivers that count (dependency), [9:12) s1 - 1, [12] / [15] prop > 0 towards s1 / s1 % 8 + 1, [13] the cell has an
// angle, [16:24) neighbours that send flow to the cell (they wait for it)
static __global__ __launch_bounds__(256) void rev_setup_kernel(const uint8_t* __restrict__ code, int nx, int ny, uint32_t* __restrict__ info) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= nx || y >= ny) return;
    unsigned c[9];
    dinf_code_window(code, nx, ny, x, y, c);   // (codes: pass 1, dinf_prop.hpp - two fp64 divisions per cell instead of ten)
    unsigned inf = 0;
    if (c[0] != DINF_CODE_NODATA) {
        inf |= d8sweep::INFO_PART | ((c[0] & 7u) << 9);
        const int s1 = int(c[0] & 7u) + 1, s2 = s1 % 8 + 1;
        // receivers that count: prop > 0, inside the raster, with an angle (src/DinfRevAccum.cpp:141-150)
        unsigned has_angle = 0;   // bit k - 1: neighbour k lies in the raster and has an angle
#pragma unroll
        for (int k = 1; k <= 8; k++) has_angle |= (c[k] != DINF_CODE_NODATA) ? 1u << (k - 1) : 0u;
        if (c[0] & DINF_CODE_P1) inf |= RINFO_P1 | (has_angle & (1u << (s1 - 1)));
        if (c[0] & DINF_CODE_P2) inf |= RINFO_P2 | (has_angle & (1u << (s2 - 1)));
        // who waits for this cell: neighbours with an angle whose flow reaches it (only meaningful when the cell itself has an angle:
        // a receiver without one is not counted by its senders)
#pragma unroll
        for (int k = 1; k <= 8; k++) {
            const int kk = (k + 4) % 8;
            if (dinf_code_sends(c[k], kk == 0 ? 8 : kk)) inf |= 1u << (16 + k - 1);
        }
    }
    info[size_t(y) * size_t(nx) + size_t(x)] = inf;
}

// the two receiver directions in ascending k (the reference's loop order), with their proportion slots
struct Recv { int k[2]; bool on[2]; };
__device__ __forceinline__ Recv receivers(unsigned inf) {
    const int s1 = int((inf >> 9) & 7u) + 1, s2 = s1 % 8 + 1;
    Recv r;
    const bool p1 = (inf & RINFO_P1) != 0u, p2 = (inf & RINFO_P2) != 0u;
    if (s2 > s1) { r.k[0] = s1; r.on[0] = p1; r.k[1] = s2; r.on[1] = p2; }
    else { r.k[0] = s2; r.on[0] = p2; r.k[1] = s1; r.on[1] = p1; }   // s1 == 8: k = 1 is visited before k = 8
    return r;
}

// what a pending cell needs in the lockstep form of the reverse sweep (d8sweep::sweep_tile_rev), made once per activation: its receivers
// in ascending k, which of them count (prop > 0, inside the raster, with an angle) and their proportions
__device__ __forceinline__ void rev_row_dinf(unsigned inf, float angle, double a2, int (&k)[2], bool (&on)[2], double (&p)[2]) {
    const Recv r = receivers(inf);
#pragma unroll
    for (int t = 0; t < 2; t++) {
        k[t] = r.k[t];
        on[t] = r.on[t] && ((inf >> (r.k[t] - 1)) & 1u) != 0u;
        p[t] = on[t] ? prop_dev(angle, r.k[t], a2) : 0.;
    }
}

static __global__ __launch_bounds__(256) void rev_init2_kernel(const uint32_t* __restrict__ info, float2* __restrict__ rec, size_t first, size_t n) {
    const size_t i = first + size_t(blockIdx.x) * 256 + threadIdx.x;
    if (i < first + n) rec[i] = (info[i] & d8sweep::INFO_PART) ? make_float2(__uint_as_float(d8sweep::PENDING_BITS), 0.f) : make_float2(TDX_ANG_NODATA, TDX_ANG_NODATA);
}
static __global__ __launch_bounds__(256) void rev_unpack2_kernel(const float2* __restrict__ rec, size_t first, size_t n, float* __restrict__ racc, float* __restrict__ dmax) {
    const size_t i = first + size_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= first + n) return;
    const float2 r = rec[i];
    const bool pend = d8sweep::pending(r.x);   // on or above a cycle: never queued by the reference either
    racc[i] = pend ? TDX_ANG_NODATA : r.x;
    dmax[i] = pend ? TDX_ANG_NODATA : r.y;
}

struct RevSetup {
    double* d_a2 = nullptr;
    uint32_t* info = nullptr;
    float2* aux = nullptr;
    uint32_t* flags = nullptr;
    unsigned long long* counts = nullptr;
};
// common front part: halo rows of the angle grid, per-row atan2 table, info words
static int rev_prepare(tdx_context* ctx, const Strip& st, float* d_ang, float ang_nodata, const double* dxc, const double* dyc, RevSetup& R, tdx_stats* stats,
                       const char* stage = "dinfupdependence / dinfrevaccum") {
    hipStream_t s = ctx->stream;
    const int inx = st.nx, iny = st.ny_arr;
    const size_t n = size_t(inx) * size_t(iny);
    std::vector<double> a2(size_t(iny), 0.);
    for (int j = 0; j < iny; j++) a2[size_t(j)] = atan2(dyc[j], dxc[j]);
    const tilek::TileGeom geom = tilek::make_geom(inx, iny, st.y0, st.y1);
    const size_t ntiles = size_t(geom.tiles_x) * size_t(geom.tiles_y);
    R.d_a2 = static_cast<double*>(ctx->scratch(TDX_S_J, a2.size() * 8));
    R.info = static_cast<uint32_t*>(ctx->scratch(TDX_S_A, n * 4));
    R.aux = static_cast<float2*>(ctx->scratch(TDX_S_B, n * 8));
    R.flags = static_cast<uint32_t*>(ctx->scratch(TDX_S_L, ntiles * 4 * (1 + tilek::SCHED_LIST_WORDS)));
    R.counts = static_cast<unsigned long long*>(ctx->scratch(TDX_S_M, size_t(tilek::COUNT_RING) * 16));
    if (!R.d_a2 || !R.info || !R.aux || !R.flags || !R.counts) return TDX_ERR_NOMEM;
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(R.d_a2, a2.data(), a2.size() * 8, hipMemcpyHostToDevice, s));
    TDX_HIP_CHECK(ctx, hipStreamSynchronize(s));   // `a2` is a local
    ctx->begin_call(stats);
    strip_mark(ctx, st, stage);
    int rc = strip_exchange<float>(ctx, st, d_ang, ang_nodata);   // flowData->share()
    if (rc != TDX_OK) return rc;
    TdxSpan sp(ctx, TDX_K_STENCIL);
    uint8_t* code = static_cast<uint8_t*>(ctx->scratch(TDX_S_D, n));
    if (!code) return TDX_ERR_NOMEM;
    hipLaunchKernelGGL(dinf_code_kernel, dim3(tdx_blocks_for(n, 256)), dim3(256), 0, s, d_ang, n, inx, ang_nodata, -1.0e30f, R.d_a2, code);   // (no outlets mode here)
    hipLaunchKernelGGL(rev_setup_kernel, dim3((inx + 63) / 64, (iny + 3) / 4), dim3(256), 0, s, code, inx, iny, R.info);
    if (stats) stats->launches[TDX_K_STENCIL]++;
    return TDX_OK;
}

}  // namespace dinfrev
