// PeukerDouglas (src/PeukerDouglas.cpp:54-241): the stream-source raster of the curvature-based stream definition.  The reference smooths the elevations
// with a weighted 3x3 kernel (:109-155), then scans overlapping 2x2 groups of the smoothed grid and unflags, per group, the highest cell, every cell equal
// to it and - when a cell of the group is nodata - all four (:168-212).  The scan only ever CLEARS flags, so the result is the initial mask minus the union
// of what each group clears: every cell is a function of the 3x3 smoothed window around it, i.e. of a 5x5 window of the input.
//
//   peuker_fused_kernel    fel -> ss [, w] in one streaming pass: a lane walks down a column segment with the raw rows, the smoothed rows and the
//                          groups' clear masks in registers; west / east values are DPP lane shifts, so a wave yields 60 output columns of its 64
//                          lanes (two columns of overlap each side: one for the smoothing, one for the groups).  4 B read, 2 B written per cell
//                          (+4 B with the float copy w); no LDS, no atomics.
//   peuker_smooth_kernel,  the two passes apart, with the smoothed grid in scratch between them: what a row strip needs (the smoothed edge rows of the
//   peuker_flag_kernel     neighbouring strips are exchanged in between - the reference's second share()), and the A/B baseline of the fused pass
//                          on one device (TDX_PEUKER_TWOPASS=1).
//
// Only cells that are not on the raster's rim can be flagged, and such a cell's four groups lie inside the raster: nothing outside the raster is ever
// looked at for a cell that can be 1, so rows and columns beyond it are only clamped into the array.
#include <cstdlib>

#include "context.hpp"
#include "device_common.hpp"
#include "strips.hpp"
#include "tile_relax.hpp"

namespace {

using namespace tdxk;

constexpr int PK_SEG = 32;    // rows per lane segment: 36 row loads for 32 output rows
constexpr int PK_COLS = 60;   // output columns per wave (and per block: the four waves of a block are four segments of the same columns)
constexpr int PK_NO_ROW = -0x40000000;   // "the raster's first / last row is not in this array"

// the weighted mean of src/PeukerDouglas.cpp:131-151, float, no contraction: centre, then sides 1 3 5 7 (E N W S), then diagonals 2 4 6 8 (NE NW SW SE);
// nd: bit k-1 set = neighbour k is nodata
__device__ __forceinline__ float pk_smooth(float c, float e, float ne, float n, float nw, float w, float sw, float s, float se, unsigned nd, float p0, float p1,
                                           float p2) {
    float sum = p0 * c, wsum = p0;
    if (p1 > 0.f) {
        if (!(nd & 0x01u)) { sum += e * p1; wsum += p1; }
        if (!(nd & 0x04u)) { sum += n * p1; wsum += p1; }
        if (!(nd & 0x10u)) { sum += w * p1; wsum += p1; }
        if (!(nd & 0x40u)) { sum += s * p1; wsum += p1; }
    }
    if (p2 > 0.f) {
        if (!(nd & 0x02u)) { sum += ne * p2; wsum += p2; }
        if (!(nd & 0x08u)) { sum += nw * p2; wsum += p2; }
        if (!(nd & 0x20u)) { sum += sw * p2; wsum += p2; }
        if (!(nd & 0x80u)) { sum += se * p2; wsum += p2; }
    }
    return sum / wsum;
}

// What the group c0 c1 / c2 c3 of smoothed values clears, bit m = cell m (src/PeukerDouglas.cpp:171-209).  c0 is never tested for nodata: it starts
// emax whatever it holds.  n1..n3: c1..c3 are nodata - then all four are cleared.  Otherwise the running maximum (strict '>', in the order c1 c2 c3; a
// NaN is never greater) and every cell equal to it.
__device__ __forceinline__ unsigned pk_group(float s0, float s1, float s2, float s3, bool n1, bool n2, bool n3) {
    float emax = s0;
    unsigned m = 1u;
    if (s1 > emax) { emax = s1; m = 2u; }
    if (s2 > emax) { emax = s2; m = 4u; }
    if (s3 > emax) { emax = s3; m = 8u; }
    m |= (s0 == emax ? 1u : 0u) | (s1 == emax ? 2u : 0u) | (s2 == emax ? 4u : 0u) | (s3 == emax ? 8u : 0u);
    return (n1 || n2 || n3) ? 15u : m;
}

// The value the lane to the west / east holds; lane 0 / lane 63 get 0.  (tilek::lane_left / lane_right with bound_ctrl instead of an edge value: the
// move needs no register preset with the edge, and every edge of this kernel is 0 - lanes 0 and 63 are never output lanes.)
template <class T>
__device__ __forceinline__ T pk_west(T x) {
    static_assert(sizeof(T) == 4, "32-bit values");
    return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), tilek::DPP_WAVE_SHR1, 0xf, 0xf, true));
}
template <class T>
__device__ __forceinline__ T pk_east(T x) {
    static_assert(sizeof(T) == 4, "32-bit values");
    return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), tilek::DPP_WAVE_SHL1, 0xf, 0xf, true));
}
__device__ __forceinline__ unsigned long long pk_east64(unsigned long long v) { return ((unsigned long long)pk_east(unsigned(v >> 32)) << 32) | (unsigned long long)pk_east(unsigned(v)); }

// Lane lx of a wave holds column bx * 60 - 2 + lx.  Raw values are right in every lane, smoothed values in lanes 1..62 (they need both neighbours), the
// groups with origin in this column in lanes 1..61 (they need the smoothed column to the east), the flags in lanes 2..61 (they need the groups of the column
// to the west).  What the other lanes compute is never stored.
template <int SEG>
__global__ __launch_bounds__(256) void peuker_fused_kernel(const float* __restrict__ Z, int nx, int ny, float nodata, float p0, float p1, float p2,
                                                           int16_t* __restrict__ SS, float* __restrict__ WF, int nbx, int xmap) {
    const int bx = tdxk::xcd_block_x(nbx, xmap);
    if (bx < 0) return;
    const int lx = threadIdx.x & 63;
    const int x = bx * PK_COLS - 2 + lx;
    const int band = __builtin_amdgcn_readfirstlane(int(blockIdx.y) * 4 + int(threadIdx.x >> 6));
    const int ybase = band * SEG;
    if (ybase >= ny) return;   // (wave-uniform; the kernel has no barrier)
    const bool mine = lx >= 2 && lx < 2 + PK_COLS && x < nx;
    const bool xrim = x <= 0 || x >= nx - 1;
    const int xc = x < 0 ? 0 : (x >= nx ? nx - 1 : x);
    // raw rows ybase - 2 .. ybase + SEG + 1, clamped into the array, all loads issued back to back
    float z[SEG + 4];
#pragma unroll
    for (int j = 0; j < SEG + 4; j++) {
        const int y = ybase - 2 + j, yc = y < 0 ? 0 : (y >= ny ? ny - 1 : y);
        z[j] = Z[size_t(yc) * size_t(nx) + size_t(xc)];
    }
    unsigned long long ndz = 0;   // bit j: raw row j of this column is nodata
#pragma unroll
    for (int j = 0; j < SEG + 4; j++)
        if (is_nodata_f(z[j], nodata)) ndz |= 1ull << j;
    // What each loaded value adds to a neighbour's weighted sum (a) and weight sum (b), as a side cell (1) and as a diagonal cell (2), formed once per
    // value: nothing when it is nodata or when its group's weight is not > 0.  Where the reference skips a cell, 0.f is added instead, which leaves the
    // running float sums as they are (a sum of -0 becomes +0; no comparison downstream tells the two apart, and 0 / 0 is NaN either way) - so the
    // terms below are the reference's, in its order: centre, sides 1 3 5 7 (E N W S), diagonals 2 4 6 8 (NE NW SW SE).
    // The columns beside this one come by lane shifts.  Like every lane shift of this kernel these are made outside any branch that differs between
    // lanes: a DPP move does not read a lane that a divergent branch has switched off.
    const bool use1 = p1 > 0.f, use2 = p2 > 0.f;
    float a1[SEG + 4], a2[SEG + 4], b1[SEG + 4], b2[SEG + 4];
#pragma unroll
    for (int j = 0; j < SEG + 4; j++) {
        const bool nd = (ndz >> j) & 1ull;
        a1[j] = (nd || !use1) ? 0.f : z[j] * p1;
        b1[j] = (nd || !use1) ? 0.f : p1;
        a2[j] = (nd || !use2) ? 0.f : z[j] * p2;
        b2[j] = (nd || !use2) ? 0.f : p2;
    }
    // smoothed rows ybase - 1 .. ybase + SEG: row j is centred on raw row j + 1
    float s[SEG + 2];
    unsigned long long nds = 0;   // bit j: smoothed row j of this column is nodata
#pragma unroll
    for (int j = 0; j < SEG + 2; j++) {
        const int y = ybase - 1 + j;
        const float c = z[j + 1];
        const bool copied = xrim || y <= 0 || y >= ny - 1 || ((ndz >> (j + 1)) & 1ull);
        float sum = p0 * c, wsum = p0;
        sum += pk_east(a1[j + 1]); wsum += pk_east(b1[j + 1]);
        sum += a1[j];                      wsum += b1[j];
        sum += pk_west(a1[j + 1]);  wsum += pk_west(b1[j + 1]);
        sum += a1[j + 2];                  wsum += b1[j + 2];
        sum += pk_east(a2[j]);     wsum += pk_east(b2[j]);
        sum += pk_west(a2[j]);      wsum += pk_west(b2[j]);
        sum += pk_west(a2[j + 2]);  wsum += pk_west(b2[j + 2]);
        sum += pk_east(a2[j + 2]); wsum += pk_east(b2[j + 2]);
        const float v = copied ? c : sum / wsum;
        s[j] = v;
        if (is_nodata_f(v, nodata)) nds |= 1ull << j;
    }
    const unsigned long long ndse = pk_east64(nds);
    // groups with origin rows ybase - 1 .. ybase + SEG - 1, eight 4-bit masks to a word
    unsigned gp[(SEG + 1 + 7) / 8] = {};
    float se0 = pk_east(s[0]);
#pragma unroll
    for (int j = 0; j < SEG + 1; j++) {
        const float se1 = pk_east(s[j + 1]);
        const unsigned g = pk_group(s[j], se0, s[j + 1], se1, (ndse >> j) & 1ull, (nds >> (j + 1)) & 1ull, (ndse >> (j + 1)) & 1ull);
        gp[j >> 3] |= g << (4 * (j & 7));
        se0 = se1;
    }
    unsigned gw[(SEG + 1 + 7) / 8];
#pragma unroll
    for (int k = 0; k < (SEG + 1 + 7) / 8; k++) gw[k] = pk_west(gp[k]);
    if (!mine) return;
#pragma unroll
    for (int r = 0; r < SEG; r++) {
        const int y = ybase + r;
        if (y >= ny) break;
        // the cell is c3 of the group north-west of it, c2 of the one north, c1 of the one west and c0 of its own
        const unsigned cleared = ((gw[r >> 3] >> (4 * (r & 7))) & 8u) | ((gp[r >> 3] >> (4 * (r & 7))) & 4u) | ((gw[(r + 1) >> 3] >> (4 * ((r + 1) & 7))) & 2u) |
                                 ((gp[(r + 1) >> 3] >> (4 * ((r + 1) & 7))) & 1u);
        const int flag = (!xrim && y >= 1 && y <= ny - 2 && cleared == 0u) ? 1 : 0;
        const size_t idx = size_t(y) * size_t(nx) + size_t(x);
        SS[idx] = int16_t(flag);
        if (WF) WF[idx] = float(flag);
    }
}

// the smoothed grid of the owned rows [y0, y1) of an array of ny_arr rows; gtop / gbot: the array rows that are the raster's first / last row
__global__ __launch_bounds__(256) void peuker_smooth_kernel(const float* __restrict__ Z, int nx, int ny_arr, int y0, int y1, int gtop, int gbot, float nodata, float p0,
                                                            float p1, float p2, float* __restrict__ S) {
    const unsigned long long q = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (q >= (unsigned long long)(y1 - y0) * (unsigned long long)nx) return;
    const int y = y0 + int(q / (unsigned long long)nx), x = int(q % (unsigned long long)nx);
    const size_t idx = size_t(y) * size_t(nx) + size_t(x);
    const float c = Z[idx];
    float v = c;
    if (!(x == 0 || x == nx - 1 || y == gtop || y == gbot || y <= 0 || y >= ny_arr - 1 || is_nodata_f(c, nodata))) {
        const float* zn = Z + idx - size_t(nx);
        const float* zs = Z + idx + size_t(nx);
        const float e = Z[idx + 1], ne = zn[1], n = zn[0], nw = zn[-1], w = Z[idx - 1], sw = zs[-1], s = zs[0], se = zs[1];
        const unsigned nd = (is_nodata_f(e, nodata) ? 1u : 0u) | (is_nodata_f(ne, nodata) ? 2u : 0u) | (is_nodata_f(n, nodata) ? 4u : 0u) |
                            (is_nodata_f(nw, nodata) ? 8u : 0u) | (is_nodata_f(w, nodata) ? 16u : 0u) | (is_nodata_f(sw, nodata) ? 32u : 0u) |
                            (is_nodata_f(s, nodata) ? 64u : 0u) | (is_nodata_f(se, nodata) ? 128u : 0u);
        v = pk_smooth(c, e, ne, n, nw, w, sw, s, se, nd, p0, p1, p2);
    }
    S[idx] = v;
}

// the flags of the owned rows from the smoothed grid (rows y0 - 1 and y1 of it are the neighbouring strips' edge rows, or anything at all beyond the raster)
__global__ __launch_bounds__(256) void peuker_flag_kernel(const float* __restrict__ S, int nx, int ny_arr, int y0, int y1, int gtop, int gbot, float nodata,
                                                          int16_t* __restrict__ SS, float* __restrict__ WF) {
    const unsigned long long q = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (q >= (unsigned long long)(y1 - y0) * (unsigned long long)nx) return;
    const int y = y0 + int(q / (unsigned long long)nx), x = int(q % (unsigned long long)nx);
    const size_t idx = size_t(y) * size_t(nx) + size_t(x);
    int flag = 0;
    if (!(x == 0 || x == nx - 1 || y == gtop || y == gbot || y <= 0 || y >= ny_arr - 1)) {
        float v[3][3];
        bool nd[3][3];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                v[i][j] = S[idx + size_t(nx) * size_t(i) + size_t(j) - size_t(nx) - 1];
                nd[i][j] = is_nodata_f(v[i][j], nodata);
            }
        const unsigned cleared = (pk_group(v[0][0], v[0][1], v[1][0], v[1][1], nd[0][1], nd[1][0], nd[1][1]) & 8u) |
                                 (pk_group(v[0][1], v[0][2], v[1][1], v[1][2], nd[0][2], nd[1][1], nd[1][2]) & 4u) |
                                 (pk_group(v[1][0], v[1][1], v[2][0], v[2][1], nd[1][1], nd[2][0], nd[2][1]) & 2u) |
                                 (pk_group(v[1][1], v[1][2], v[2][1], v[2][2], nd[1][2], nd[2][1], nd[2][2]) & 1u);
        flag = cleared == 0u ? 1 : 0;
    }
    SS[idx] = int16_t(flag);
    if (WF) WF[idx] = float(flag);
}

// One strip (or the whole raster, a strip without halo rows).  fused: the single pass; it has no halo rows to read, so only for a whole raster.
int peuker_impl(tdx_context* ctx, const Strip& st, float* d_fel, float nodata, float p0, float p1, float p2, int16_t* d_ss, float* d_w, tdx_stats* stats, bool fused) {
    TDX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const bool whole = st.ny_arr == st.y1 - st.y0;
    float* d_s = nullptr;
    if (!(fused && whole)) {
        d_s = static_cast<float*>(ctx->scratch(TDX_S_A, size_t(st.nx) * size_t(st.ny_arr) * sizeof(float)));
        if (!d_s) return TDX_ERR_NOMEM;
    }
    ctx->begin_call(stats);
    strip_mark(ctx, st, "peukerdouglas");
    if (fused && whole) {
        ctx->phase = "fused pass";
        TdxSpan sp(ctx, TDX_K_STENCIL);
        const int nbx = (st.nx + PK_COLS - 1) / PK_COLS, nband4 = (st.ny_arr + 4 * PK_SEG - 1) / (4 * PK_SEG);
        hipLaunchKernelGGL(peuker_fused_kernel<PK_SEG>, dim3(tdx_xcd_grid_x(unsigned(nbx)), unsigned(nband4)), dim3(256), 0, s, d_fel, st.nx, st.ny_arr, nodata, p0, p1, p2,
                           d_ss, d_w, nbx, tdx_xcd_map() ? 1 : 0);
        if (stats) stats->launches[TDX_K_STENCIL]++;
    } else {
        // the raster's first / last row, as rows of this array
        const int gtop = st.up ? PK_NO_ROW : st.y0, gbot = st.down ? PK_NO_ROW : st.y1 - 1;
        const unsigned grid = tdx_blocks_for(uint64_t(st.y1 - st.y0) * uint64_t(st.nx), 256);
        ctx->phase = "smoothing";
        int rc = strip_exchange<float>(ctx, st, d_fel, nodata);   // the reference's first share(): raw elevations
        if (rc != TDX_OK) return rc;
        {
            TdxSpan sp(ctx, TDX_K_STENCIL);
            hipLaunchKernelGGL(peuker_smooth_kernel, dim3(grid), dim3(256), 0, s, d_fel, st.nx, st.ny_arr, st.y0, st.y1, gtop, gbot, nodata, p0, p1, p2, d_s);
        }
        ctx->phase = "flags";
        rc = strip_exchange<float>(ctx, st, d_s, nodata);   // its second: smoothed elevations
        if (rc != TDX_OK) return rc;
        {
            TdxSpan sp(ctx, TDX_K_STENCIL);
            hipLaunchKernelGGL(peuker_flag_kernel, dim3(grid), dim3(256), 0, s, d_s, st.nx, st.ny_arr, st.y0, st.y1, gtop, gbot, nodata, d_ss, d_w);
        }
        if (stats) stats->launches[TDX_K_STENCIL] += 2;
    }
    TDX_HIP_CHECK(ctx, hipGetLastError());
    ctx->end_call();
    return TDX_OK;
}

int peuker_check(tdx_context* ctx, const void* fel, const void* ss, int64_t nx, int64_t ny, int64_t halo, const char* who) {
    if (!ctx || !fel || !ss || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, who);
    return too_big(nx, ny + halo) ? tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip") : TDX_OK;
}

}  // namespace

extern "C" int tdx_peukerdouglas_dev(tdx_context* ctx, const float* d_fel, int64_t nx, int64_t ny, float fel_nodata, float w_center, float w_side, float w_diag,
                                     int16_t* d_ss, float* d_w, tdx_stats* stats) {
    if (int rc = peuker_check(ctx, d_fel, d_ss, nx, ny, 0, "tdx_peukerdouglas_dev: bad argument")) return rc;
    const bool twopass = getenv("TDX_PEUKER_TWOPASS") != nullptr;   // (A/B hook, read per call: the two kernels with the smoothed grid in scratch)
    return peuker_impl(ctx, strip_single(int(nx), int(ny)), const_cast<float*>(d_fel), fel_nodata, w_center, w_side, w_diag, d_ss, d_w, stats, !twopass);
}

extern "C" int tdx_peukerdouglas_strip(tdx_context* ctx, const tdx_comm* comm, float* d_fel, int64_t nx, int64_t ny_local, float fel_nodata, float w_center,
                                       float w_side, float w_diag, int16_t* d_ss, float* d_w, tdx_stats* stats) {
    if (int rc = peuker_check(ctx, d_fel, d_ss, nx, ny_local, 2, "tdx_peukerdouglas_strip: bad argument")) return rc;
    return peuker_impl(ctx, strip_from_comm(comm, int(nx), int(ny_local)), d_fel, fel_nodata, w_center, w_side, w_diag, d_ss, d_w, stats, false);
}

extern "C" int tdx_peukerdouglas(tdx_context* ctx, const float* fel, int64_t nx, int64_t ny, float fel_nodata, float w_center, float w_side, float w_diag, int16_t* ss,
                                 float* w, tdx_stats* stats) {
    if (!ctx || !fel || !ss || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_peukerdouglas: bad argument");
    HostCall h(ctx, nx, ny);
    float* d_z = h.in(TDX_S_IO0, fel);
    int16_t* d_ss = h.out(TDX_S_IO1, ss);
    float* d_w = h.out(TDX_S_IO2, w);   // optional
    if (h.error) return h.error;
    return h.finish(tdx_peukerdouglas_dev(ctx, d_z, nx, ny, fel_nodata, w_center, w_side, w_diag, d_ss, d_w, stats));
}
