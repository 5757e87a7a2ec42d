// The set-up shared by the FORWARD D-infinity sweeps (dinflim.hip: DinfConcLimAccum, DinfTransLimAccum; dinfdistup.hip: DinfDistUp): the
// info words of AreaDinf's dependency graph - a cell waits for the neighbours whose flow reaches it (initNeighborDinfup,
// src/commonLib.cpp:99-131) and releases its at most two receivers - the per-row tables, the halo of the angle grid, the outlet
// recode when there are outlets, and the sweep of a policy with a 16-byte record.
#pragma once
#include <cmath>
#include <cstring>
#include <vector>

#include "context.hpp"
#include "d8_sweep.hpp"
#include "device_common.hpp"
#include "dinf_outlets.hpp"
#include "dinf_prop.hpp"

namespace dinffwd {
using namespace tdxk;

constexpr unsigned FINFO_P1 = 1u << 12, FINFO_P2 = 1u << 15;

// Per cell: [0:8) contributors (dependency and value), [8] a neighbour is missing (off the raster or without angle: edge
// contamination), [9:12) s1 - 1, [12] / [15] prop > 0 towards s1 / s1 % 8 + 1, [13] the cell participates
static __global__ __launch_bounds__(256) void fwd_setup_kernel(const uint8_t* __restrict__ code, int nx, int ny, uint32_t* __restrict__ info) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= nx || y >= ny) return;
    unsigned c[9];
    dinf_code_window(code, nx, ny, x, y, c);   // (codes: pass 1, dinf_prop.hpp - two fp64 divisions per cell instead of ten)
    unsigned inf = 0;
#pragma unroll
    for (int k = 1; k <= 8; k++) {
        if (dinf_code_missing(c[k])) inf |= d8sweep::INFO_CON;   // (a sink on a cell without angle: missing for the contamination test, sends nothing)
        if (c[k] == DINF_CODE_NODATA) continue;
        const int kk = (k + 4) % 8;
        if (dinf_code_sends(c[k], kk == 0 ? 8 : kk)) inf |= 1u << (k - 1);   // `float p > 0` of src/commonLib.cpp:99 == the sender's own proportion > 0
    }
    if (c[0] != DINF_CODE_NODATA && (c[0] & DINF_CODE_PART)) {
        inf |= d8sweep::INFO_PART | ((c[0] & 7u) << 9);
        if (c[0] & DINF_CODE_P1) inf |= FINFO_P1;
        if (c[0] & DINF_CODE_P2) inf |= FINFO_P2;
    }
    info[size_t(y) * size_t(nx) + size_t(x)] = inf;
}
__device__ __forceinline__ unsigned fwd_rel_mask(unsigned inf) {
    const int s1 = int((inf >> 9) & 7u) + 1, s2 = s1 % 8 + 1;
    return ((inf & FINFO_P1) ? 1u << (s1 - 1) : 0u) | ((inf & FINFO_P2) ? 1u << (s2 - 1) : 0u);
}

struct FwdSetup {
    RowProp* d_rows = nullptr;
    double* d_a2 = nullptr;
    uint32_t* info = nullptr;
    float4* rec = nullptr;
    uint32_t* flags = nullptr;
    unsigned long long* counts = nullptr;
    float* ang_use = nullptr;
};
// common front part: halo rows of the angle grid, per-row tables, outlets, info words.  `stage` names the caller (strip_mark); n_outlets < 0
// skips the outlet recode (the sweep then runs on d_ang itself: R.ang_use == d_ang)
static int fwd_prepare(tdx_context* ctx, const Strip& st, float* d_ang, float ang_nodata, const double* dxc, const double* dyc, const int32_t* outlet_x,
                       const int32_t* outlet_y, int64_t n_outlets, FwdSetup& R, tdx_stats* stats, const char* stage = "dinfconclimaccum / dinftranslimaccum") {
    if (n_outlets > 0 && (!outlet_x || !outlet_y)) return tdx_fail(ctx, TDX_ERR_ARG, "outlets missing");
    hipStream_t s = ctx->stream;
    const int inx = st.nx, iny = st.ny_arr;
    const size_t n = size_t(inx) * size_t(iny);
    std::vector<RowProp> rows(static_cast<size_t>(iny));
    std::vector<double> a2(static_cast<size_t>(iny));
    for (int j = 0; j < iny; j++) { a2[size_t(j)] = atan2(dyc[j], dxc[j]); rows[size_t(j)].a2 = a2[size_t(j)]; rows[size_t(j)].dx = dxc[j]; }
    const tilek::TileGeom geom = tilek::make_geom(inx, iny, st.y0, st.y1);
    const size_t ntiles = size_t(geom.tiles_x) * size_t(geom.tiles_y);
    R.d_rows = static_cast<RowProp*>(ctx->scratch(TDX_S_J, rows.size() * sizeof(RowProp)));
    R.d_a2 = static_cast<double*>(ctx->scratch(TDX_S_K, a2.size() * 8));
    R.info = static_cast<uint32_t*>(ctx->scratch(TDX_S_A, n * 4));
    R.rec = static_cast<float4*>(ctx->scratch(TDX_S_C, n * 16));
    R.counts = static_cast<unsigned long long*>(ctx->scratch(TDX_S_M, size_t(tilek::COUNT_RING) * 16));
    if (!R.d_rows || !R.d_a2 || !R.info || !R.rec || !R.counts) return TDX_ERR_NOMEM;
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(R.d_rows, rows.data(), rows.size() * sizeof(RowProp), hipMemcpyHostToDevice, s));
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(R.d_a2, a2.data(), a2.size() * 8, hipMemcpyHostToDevice, s));
    TDX_HIP_CHECK(ctx, hipStreamSynchronize(s));   // the tables are locals
    ctx->begin_call(stats);
    strip_mark(ctx, st, stage);
    int rc = strip_exchange<float>(ctx, st, d_ang, ang_nodata);   // flowData->share()
    if (rc != TDX_OK) return rc;
    R.ang_use = d_ang;
    if (n_outlets >= 0) {
        rc = dinf_outlet_recode(ctx, st, d_ang, ang_nodata, R.d_rows, outlet_x, outlet_y, n_outlets, &R.ang_use, stats);
        if (rc != TDX_OK) return rc;
    }
    R.flags = static_cast<uint32_t*>(ctx->scratch(TDX_S_L, ntiles * 4 * (1 + tilek::SCHED_LIST_WORDS)));   // (after the closure, which uses the same slot)
    if (!R.flags) return TDX_ERR_NOMEM;
    TdxSpan sp(ctx, TDX_K_STENCIL);
    uint8_t* code = static_cast<uint8_t*>(ctx->scratch(TDX_S_D, n));
    if (!code) return TDX_ERR_NOMEM;
    hipLaunchKernelGGL(dinf_code_kernel, dim3(tdx_blocks_for(n, 256)), dim3(256), 0, s, R.ang_use, n, inx, ang_nodata, TDX_ANG_OUTSIDE, R.d_a2, code);
    hipLaunchKernelGGL(fwd_setup_kernel, dim3((inx + 63) / 64, (iny + 3) / 4), dim3(256), 0, s, code, inx, iny, R.info);
    if (stats) stats->launches[TDX_K_STENCIL]++;
    return TDX_OK;
}

// the forward sweep of policy Alg (16-byte record) over the prepared info words; R.rec holds the packed records of the owned rows.  dist:
// the [array row][9] table of a HAS_DIST policy
template <class Alg>
int fwd_sweep(tdx_context* ctx, const Strip& st, Alg alg, FwdSetup& R, const typename Alg::Aux* aux, tdx_stats* stats, int64_t* rounds, int64_t* outer,
              const float* dist = nullptr) {
    {   // records of the neighbours' boundary rows
        const float4 oc = Alg::outside();
        uint4 ob;
        memcpy(&ob, &oc, sizeof(ob));
        int rc = strip_exchange<uint4>(ctx, st, reinterpret_cast<uint4*>(R.rec), ob);
        if (rc != TDX_OK) return rc;
    }
    int64_t launches = 0;
    TdxSpan sp(ctx, TDX_K_ACCUM);
    d8sweep::Arrays<Alg> A{R.rec, aux, dist, R.d_a2, R.info};
    int rc = d8sweep::run(ctx, st, alg, A, R.counts, rounds, &launches, outer);
    if (rc != TDX_OK) return rc;
    if (stats) stats->launches[TDX_K_ACCUM] += launches;
    return TDX_OK;
}

}  // namespace dinffwd
