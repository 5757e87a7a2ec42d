// StreamNet (netsetup, src/streamnet.cpp:372-1508) on gfx950: the stream network's link tree, its order grid and its catchment grid.
//
// The dense work of the reference is two Kahn queues over the whole raster that walk UPSTREAM, the shape of d8sweep::sweep_tile_rev (d8_sweep.hpp)
// with set-ups of its own here (the three modes of d8_rev.hpp are not touched):
//   length sweep  (:562-650)   restricted to the stream cells S = {src not nodata, src > 0, p not nodata} (:567).  A stream cell depends on its receiver
//                              only where that is a stream cell too; otherwise it is a stream end with length 0.  lengths = float(double(lengths[receiver])
//                              + step), the step a double of the cell's own row (dxc, dyc or sqrt(dxc^2 + dyc^2): :604-606), rounded once per cell; one
//                              receiver per cell, so the bits do not depend on the schedule.  A p == 0 stream cell names itself as receiver and waits for
//                              ever (INFO_DEAD), with everything above it: MISSINGFLOAT.
//   label sweep   (:1347-1441) over the cells with a direction that are OFF the stream by src (src nodata or < 1): a cell takes the record of its receiver.
//                              The records of all other cells are final before the sweep starts - the stream cells carry the link builder's wsGrid (nodata
//                              where the walk never came), a cell "on stream" by src without a direction carries nodata and passes it on - so "the
//                              receiver has src >= 1" of the reference's seeds is simply "the receiver's record is not pending".
// Between them the stream cells are compacted in row-major order (a block scan and a scan of the block totals; a rank grid and one gather give each cell
// the compact rank of its receiver), the host builds the links over the compact arrays (streamnet_links.cpp: the reference's FIFO and its link numbers
// are sequential by definition, and touch ~1 % of the cells), and the per-cell labels and orders are scattered back.  That is the default.  The
// _gpu_links entry points build the links on the device instead (streamnet_links_device.hip: the queue's order has a closed form): the compact columns
// stay where gather_kernel left them, the labels and orders are scattered from where the builder wrote them, and only the tree and coord rows come down.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "context.hpp"
#include "d8_rev.hpp"
#include "d8_sweep.hpp"
#include "device_common.hpp"
#include "streamnet_links.hpp"
#include "streamnet_links_device.hpp"

struct tdx_streamnet_links {
    streamnet::Links links;
    int64_t stream_cells = 0;
    double phase_ms[TDX_STREAMNET_PHASES] = {0, 0, 0, 0, 0, 0, 0};
    bool device_built = false;             // the links came from streamnet_links_device.hip
    streamnet::DeviceLinkStats dstats;     // its sub-phases, rounds and workspace (tdx_streamnet_links_device_phases)
};

// the stream cells of one strip's owned rows (tdx_streamnet_compact_strip), in row-major order
struct tdx_streamnet_compact {
    int64_t nx = 0, row_shift = 0;       // global row = array row + row_shift
    std::vector<uint32_t> cidx;          // index in the strip array
    std::vector<int16_t> p;
    std::vector<float> fel, ad8, len;
    std::vector<int32_t> recv;           // rank of the receiver among the stream cells of the strip that owns it, -1: not a stream cell
    std::vector<int8_t> recv_strip;      // that strip: -1 the one above, 0 this one, +1 the one below
    std::vector<uint8_t> flags;
};

namespace {
using namespace tdxk;
using d8rev::GW_NODATA;

__device__ __forceinline__ bool src_pos(const int32_t* __restrict__ src, size_t idx, int32_t src_nodata) { return src[idx] != src_nodata && src[idx] > 0; }

struct StreamLenAlg {   // src/streamnet.cpp:595-608
    using Cell = float;
    using Aux = double;                             // the cell's own step (0 without a receiver on the stream)
    static constexpr bool HAS_AUX = true, HAS_DIST = false, HAS_ROWS = false;
    static constexpr int kBulkSweeps = 0;
    static constexpr unsigned kBulkUntil = 64;
    static constexpr int kMinWaves32 = 4;
    static constexpr int kMaxRelease = 8;
    static __device__ __forceinline__ float head(float c) { return c; }
    static __host__ __device__ __forceinline__ float outside() { return TDX_ANG_NODATA; }
    static __device__ __forceinline__ unsigned rel_mask(unsigned inf) { return (inf >> 16) & 0xFFu; }
    static __device__ __forceinline__ void rev_row(unsigned inf, const Aux&, double, int (&k)[2], bool (&on)[2], double (&p)[2]) { d8rev::rev_row_d8(inf, k, on, p); }
    __device__ __forceinline__ Cell eval2(const Aux& a, const bool (&on)[2], const double (&)[2], const Cell (&n)[2]) const {
        return on[0] ? float(double(n[0]) + a) : 0.0f;
    }
    template <class L>
    __device__ __forceinline__ void eval(L& S, int c, int cl, int, unsigned inf, const Cell (&nb)[9]) const {
        int k[2];
        bool on[2];
        double p[2];
        d8rev::rev_row_d8(inf, k, on, p);
        Cell n[2] = {0.f, 0.f};
#pragma unroll
        for (int kk = 1; kk <= 8; kk++) if (kk == k[0]) n[0] = nb[kk];
        S.v[cl] = eval2(S.aux[c], on, p, n);
    }
};

// release mask of a cell: the neighbours whose code 1..8 points at it (a superset of the sweep's senders: the mask only says which neighbouring tile looks again)
__device__ __forceinline__ unsigned senders(const int16_t* __restrict__ P, int x, int y, int nx, int ny, int16_t nodata) {
    unsigned m = 0;
#pragma unroll
    for (int k = 1; k <= 8; k++) {
        const int xn = x + d1(k), yn = y + d2(k);
        if (xn < 0 || xn >= nx || yn < 0 || yn >= ny) continue;
        const int16_t pn = P[size_t(yn) * size_t(nx) + size_t(xn)];
        if (is_nodata_s(pn, nodata) || pn < 1 || pn > 8) continue;
        if (pn - k == 4 || pn - k == -4) m |= 1u << (16 + k - 1);
    }
    return m;
}

// step9: [row][9] doubles, the step of code k on that row
__global__ __launch_bounds__(256) void len_setup_kernel(const int16_t* __restrict__ P, const int32_t* __restrict__ src, int nx, int ny, int16_t nodata, int32_t src_nodata,
                                                        const double* __restrict__ step9, uint32_t* __restrict__ info, double* __restrict__ step) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= nx || y >= ny) return;
    const size_t idx = size_t(y) * size_t(nx) + size_t(x);
    const int16_t p = P[idx];
    unsigned inf = 0;
    double stp = 0.;
    if (!is_nodata_s(p, nodata) && src_pos(src, idx, src_nodata)) {
        inf = d8sweep::INFO_PART | senders(P, x, y, nx, ny, nodata);
        if (p == 0) inf |= d8sweep::INFO_DEAD;   // its own receiver: never ready
        else if (p >= 1 && p <= 8) {
            const int xr = x + d1(p), yr = y + d2(p);
            if (xr >= 0 && xr < nx && yr >= 0 && yr < ny) {
                const size_t r = size_t(yr) * size_t(nx) + size_t(xr);
                if (!is_nodata_s(P[r], nodata) && src_pos(src, r, src_nodata)) { inf |= 1u << (p - 1); stp = step9[size_t(y) * 9 + size_t(p)]; }
            }
        }
    }
    info[idx] = inf;
    step[idx] = stp;
}

// ---- compaction: CELLS consecutive cells per thread, so that ranks follow the row-major order
constexpr int CELLS = 8, BLOCK_CELLS = 256 * CELLS;

__device__ __forceinline__ unsigned thread_mask(const int16_t* __restrict__ P, const int32_t* __restrict__ src, size_t base, size_t n, int16_t nodata, int32_t src_nodata) {
    unsigned m = 0;
#pragma unroll
    for (int i = 0; i < CELLS; i++) {
        const size_t c = base + size_t(i);
        if (c < n && !is_nodata_s(P[c], nodata) && src_pos(src, c, src_nodata)) m |= 1u << i;
    }
    return m;
}
// exclusive prefix of `c` over the 256 threads of the block; *total: the block's sum
__device__ __forceinline__ unsigned block_scan(unsigned c, unsigned* total) {
    __shared__ unsigned s_wave[4];
    const int lane = int(threadIdx.x & 63), w = int(threadIdx.x >> 6);
    unsigned v = c;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned t = __shfl_up(v, off, 64);
        if (lane >= off) v += t;
    }
    if (lane == 63) s_wave[w] = v;
    __syncthreads();
    unsigned wave_off = 0;
    for (int i = 0; i < w; i++) wave_off += s_wave[i];
    *total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    return wave_off + (v - c);
}
__global__ __launch_bounds__(256) void count_kernel(const int16_t* __restrict__ P, const int32_t* __restrict__ src, size_t n, int16_t nodata, int32_t src_nodata,
                                                    uint32_t* __restrict__ block_count) {
    const size_t base = size_t(blockIdx.x) * BLOCK_CELLS + size_t(threadIdx.x) * CELLS;
    unsigned total;
    block_scan(unsigned(__popc(thread_mask(P, src, base, n, nodata, src_nodata))), &total);
    if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}
// one block: block_count -> exclusive offsets in place, the sum to *total
__global__ __launch_bounds__(256) void offsets_kernel(uint32_t* __restrict__ block_count, unsigned nblocks, unsigned long long* __restrict__ total) {
    __shared__ unsigned s_carry;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (unsigned b0 = 0; b0 < nblocks; b0 += 256) {
        const unsigned b = b0 + threadIdx.x;
        const unsigned c = b < nblocks ? block_count[b] : 0u;
        unsigned chunk;
        const unsigned ex = block_scan(c, &chunk);
        const unsigned carry = s_carry;
        if (b < nblocks) block_count[b] = carry + ex;
        __syncthreads();   // everybody has read s_carry (and block_scan's words)
        if (threadIdx.x == 0) s_carry = carry + chunk;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = s_carry;
}
__global__ __launch_bounds__(256) void rank_kernel(const int16_t* __restrict__ P, const int32_t* __restrict__ src, size_t n, int16_t nodata, int32_t src_nodata,
                                                   const uint32_t* __restrict__ block_off, int32_t* __restrict__ rank, uint32_t* __restrict__ cidx, uint32_t index_base) {
    const size_t base = size_t(blockIdx.x) * BLOCK_CELLS + size_t(threadIdx.x) * CELLS;
    const unsigned m = thread_mask(P, src, base, n, nodata, src_nodata);
    unsigned total;
    unsigned r = block_off[blockIdx.x] + block_scan(unsigned(__popc(m)), &total);
#pragma unroll
    for (int i = 0; i < CELLS; i++) {
        const size_t c = base + size_t(i);
        if (c >= n) break;
        const bool s = (m >> i) & 1u;
        rank[c] = s ? int32_t(r) : -1;
        if (s) cidx[r++] = uint32_t(c) + index_base;   // (a strip compacts its owned rows: indices of the whole strip array)
    }
}
// per stream cell: its inputs, its length, the compact rank of its receiver (-1: not a stream cell) and the terminal test of :764-766
__global__ __launch_bounds__(256) void gather_kernel(const uint32_t* __restrict__ cidx, unsigned ncells, const int16_t* __restrict__ P, const int32_t* __restrict__ src,
                                                     const float* __restrict__ fel, const float* __restrict__ ad8, const float* __restrict__ len,
                                                     const int32_t* __restrict__ rank, int nx, int ny, int32_t src_nodata, int16_t* __restrict__ cp,
                                                     float* __restrict__ cfel, float* __restrict__ cad8, float* __restrict__ clen, int32_t* __restrict__ crecv,
                                                     uint8_t* __restrict__ cflag) {
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    if (i >= ncells) return;
    const size_t c = cidx[i];
    const int x = int(c % size_t(nx)), y = int(c / size_t(nx));
    const int16_t p = P[c];
    int32_t rv = -1;
    bool terminal = true;
    if (p >= 0 && p <= 8) {
        const int xr = x + d1(p), yr = y + d2(p);
        if (xr >= 0 && xr < nx && yr >= 0 && yr < ny) {
            const size_t r = size_t(yr) * size_t(nx) + size_t(xr);
            rv = rank[r];
            terminal = src[r] == src_nodata || src[r] != 1;
        }
    }
    cp[i] = p; cfel[i] = fel[c]; cad8[i] = ad8[c]; clen[i] = len[c]; crecv[i] = rv; cflag[i] = terminal ? streamnet::CELL_TERMINAL : uint8_t(0);
}

// ---- labels
// info words of the label sweep and the initial records: pending on the cells the sweep evaluates, 1 on the cells "on stream" by src with -sw, nodata elsewhere
__global__ __launch_bounds__(256) void label_setup_kernel(const int16_t* __restrict__ P, const int32_t* __restrict__ src, int nx, int ny, int16_t nodata, int32_t src_nodata,
                                                          int sw, uint32_t* __restrict__ info, int32_t* __restrict__ w) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= nx || y >= ny) return;
    const size_t idx = size_t(y) * size_t(nx) + size_t(x);
    const int16_t p = P[idx];
    const bool on_src = src_pos(src, idx, src_nodata);
    unsigned inf = 0;
    int32_t rec = (sw && on_src) ? 1 : GW_NODATA;
    if (!is_nodata_s(p, nodata) && !on_src && p >= 1 && p <= 8) {   // (p == 0 names the cell itself, which is off the stream: never reached)
        inf = d8sweep::INFO_PART | senders(P, x, y, nx, ny, nodata);
        const int xr = x + d1(p), yr = y + d2(p);
        if (xr >= 0 && xr < nx && yr >= 0 && yr < ny) { inf |= 1u << (p - 1); rec = int32_t(d8sweep::PENDING_BITS); }
    }
    info[idx] = inf;
    w[idx] = rec;
}
__global__ __launch_bounds__(256) void scatter_kernel(const uint32_t* __restrict__ cidx, unsigned ncells, const int32_t* __restrict__ label, const int16_t* __restrict__ order,
                                                      int sw, int32_t* __restrict__ w, int16_t* __restrict__ ord) {
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    if (i >= ncells) return;
    const size_t c = cidx[i];
    ord[c] = order[i];
    if (!sw) w[c] = label[i];
}
// what is still pending (on or above a cycle) is nodata; with -sw a cell "on stream" by src without a direction was only a seed (:1372 sits inside the p test)
__global__ __launch_bounds__(256) void label_finish_kernel(const int16_t* __restrict__ P, const int32_t* __restrict__ src, size_t n, int16_t nodata, int32_t src_nodata,
                                                           int sw, int32_t* __restrict__ w) {
    const size_t i = size_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    if (uint32_t(w[i]) == d8sweep::PENDING_BITS || (sw && is_nodata_s(P[i], nodata) && src_pos(src, i, src_nodata))) w[i] = GW_NODATA;
}

struct PhaseClock {
    tdx_context* ctx;
    std::chrono::steady_clock::time_point t;
    explicit PhaseClock(tdx_context* c) : ctx(c), t(std::chrono::steady_clock::now()) {}
    // the wall time since the last lap with the stream drained: every phase below ends in a read-back or starts from host data anyway
    int lap(double* ms) {
        TDX_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        const auto now = std::chrono::steady_clock::now();
        *ms = std::chrono::duration<double, std::milli>(now - t).count();
        t = now;
        return TDX_OK;
    }
};

int streamnet_impl(tdx_context* ctx, const int16_t* d_p, const int32_t* d_src, const float* d_fel, const float* d_ad8, int nx, int ny, int16_t p_nodata,
                   int32_t src_nodata, const double* dxc, const double* dyc, double dxA, double dyA, const double* gt, const int32_t* outlet_x, const int32_t* outlet_y,
                   const int32_t* outlet_id, int64_t nout, int sw, int16_t* d_ord, int32_t* d_w, tdx_streamnet_links* res, tdx_stats* stats,
                   bool device_links) {
    TDX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const Strip st = strip_single(nx, ny);
    const size_t n = size_t(nx) * size_t(ny);
    const unsigned nblocks = tdx_blocks_for(n, BLOCK_CELLS);
    uint32_t* info = static_cast<uint32_t*>(ctx->scratch(TDX_S_A, n * 4));
    double* step = static_cast<double*>(ctx->scratch(TDX_S_B, n * 8));
    float* len = static_cast<float*>(ctx->scratch(TDX_S_C, n * 4));
    int32_t* rank = static_cast<int32_t*>(ctx->scratch(TDX_S_D, n * 4));
    double* d_step9 = static_cast<double*>(ctx->scratch(TDX_S_F, size_t(ny) * 9 * 8));
    unsigned long long* counts = static_cast<unsigned long long*>(ctx->scratch(TDX_S_M, size_t(tilek::COUNT_RING) * 16));
    uint32_t* block_off = static_cast<uint32_t*>(ctx->scratch(TDX_S_I, size_t(nblocks) * 4 + 16));
    if (!info || !step || !len || !rank || !d_step9 || !counts || !block_off) return TDX_ERR_NOMEM;
    unsigned long long* d_total = reinterpret_cast<unsigned long long*>(block_off + ((size_t(nblocks) + 1) & ~size_t(1)));
    // the step of code k on row j in double: dxc, dyc, or the diagonal (src/streamnet.cpp:604-606)
    std::vector<double> step9(size_t(ny) * 9, 0.);
    for (int j = 0; j < ny; j++)
        for (int k = 1; k <= 8; k++)
            step9[size_t(j) * 9 + size_t(k)] = (k == 1 || k == 5) ? dxc[j] : (k == 3 || k == 7) ? dyc[j] : sqrt(dxc[j] * dxc[j] + dyc[j] * dyc[j]);
    ctx->begin_call(stats);
    strip_mark(ctx, st, "streamnet");
    PhaseClock clock(ctx);
    const dim3 grid2((nx + 63) / 64, (ny + 3) / 4);
    int64_t rounds = 0, launches = 0, outer = 1, rounds_label = 0, outer_label = 1;
    int rc;
    {   // ---- set-up of the length sweep
        TdxSpan sp(ctx, TDX_K_STENCIL);
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(d_step9, step9.data(), step9.size() * 8, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(len_setup_kernel, grid2, dim3(256), 0, s, d_p, d_src, nx, ny, p_nodata, src_nodata, d_step9, info, step);
        hipLaunchKernelGGL(d8sweep::init_kernel, dim3(tdx_blocks_for(n, 256)), dim3(256), 0, s, info, len, size_t(0), n, TDX_ANG_NODATA);
        if (stats) stats->launches[TDX_K_STENCIL] += 2;
    }
    if ((rc = clock.lap(&res->phase_ms[TDX_STREAMNET_SETUP])) != TDX_OK) return rc;
    {   // ---- distance to the outlet along the stream
        TdxSpan sp(ctx, TDX_K_ACCUM);
        d8sweep::Arrays<StreamLenAlg> A{len, step, nullptr, nullptr, info};
        rc = d8sweep::run(ctx, st, StreamLenAlg{}, A, counts, &rounds, &launches, &outer);
        if (rc != TDX_OK) return rc;
        hipLaunchKernelGGL(d8sweep::finish_kernel, dim3(tdx_blocks_for(n, 256)), dim3(256), 0, s, len, size_t(0), n, TDX_ANG_NODATA);
        if (stats) stats->launches[TDX_K_ACCUM] += launches + 1;
    }
    if ((rc = clock.lap(&res->phase_ms[TDX_STREAMNET_LENGTH])) != TDX_OK) return rc;
    // ---- compaction
    uint64_t ncells64 = 0;
    {
        TdxSpan sp(ctx, TDX_K_MISC);
        hipLaunchKernelGGL(count_kernel, dim3(nblocks), dim3(256), 0, s, d_p, d_src, n, p_nodata, src_nodata, block_off);
        hipLaunchKernelGGL(offsets_kernel, dim3(1), dim3(256), 0, s, block_off, nblocks, d_total);
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(ctx->h_mail + TDX_MAIL_STAGE, d_total, 8, hipMemcpyDeviceToHost, s));
        TDX_HIP_CHECK(ctx, hipStreamSynchronize(s));
        ncells64 = ctx->h_mail[TDX_MAIL_STAGE];
    }
    if (ncells64 > 0x7ffffff0ull) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_streamnet: more than 2^31 stream cells");
    const unsigned nc = unsigned(ncells64);
    const size_t ncp = (size_t(nc) + 3) & ~size_t(3);   // every compact array starts on a 4-byte boundary
    // cidx (u32), cfel, cad8, clen (f32), crecv, label (i32), cp, order (i16), cflag (u8)
    uint8_t* buf = static_cast<uint8_t*>(ctx->scratch(TDX_S_H, ncp * (6 * 4 + 2 * 2 + 1) + 64));
    if (!buf) return tdx_fail(ctx, TDX_ERR_NOMEM, "tdx_streamnet: out of device memory");
    uint32_t* cidx = reinterpret_cast<uint32_t*>(buf);
    float* cfel = reinterpret_cast<float*>(buf + ncp * 4);
    float* cad8 = reinterpret_cast<float*>(buf + ncp * 8);
    float* clen = reinterpret_cast<float*>(buf + ncp * 12);
    int32_t* crecv = reinterpret_cast<int32_t*>(buf + ncp * 16);
    int32_t* clabel = reinterpret_cast<int32_t*>(buf + ncp * 20);
    int16_t* cp = reinterpret_cast<int16_t*>(buf + ncp * 24);
    int16_t* corder = reinterpret_cast<int16_t*>(buf + ncp * 26);
    uint8_t* cflag = buf + ncp * 28;
    const unsigned nh = device_links ? 0u : nc;   // the host builder's copies of the columns
    std::vector<uint32_t> h_idx(nh);
    std::vector<int16_t> h_p(nh);
    std::vector<float> h_fel(nh), h_ad8(nh), h_len(nh);
    std::vector<int32_t> h_recv(nh);
    std::vector<uint8_t> h_flag(nh);
    {
        TdxSpan sp(ctx, TDX_K_MISC);
        hipLaunchKernelGGL(rank_kernel, dim3(nblocks), dim3(256), 0, s, d_p, d_src, n, p_nodata, src_nodata, block_off, rank, cidx, 0u);
        if (nc) {
            hipLaunchKernelGGL(gather_kernel, dim3(tdx_blocks_for(nc, 256)), dim3(256), 0, s, cidx, nc, d_p, d_src, d_fel, d_ad8, len, rank, nx, ny, src_nodata, cp, cfel,
                               cad8, clen, crecv, cflag);
        }
        if (nh) {
            TDX_HIP_CHECK(ctx, hipMemcpyAsync(h_idx.data(), cidx, size_t(nc) * 4, hipMemcpyDeviceToHost, s));
            TDX_HIP_CHECK(ctx, hipMemcpyAsync(h_p.data(), cp, size_t(nc) * 2, hipMemcpyDeviceToHost, s));
            TDX_HIP_CHECK(ctx, hipMemcpyAsync(h_fel.data(), cfel, size_t(nc) * 4, hipMemcpyDeviceToHost, s));
            TDX_HIP_CHECK(ctx, hipMemcpyAsync(h_ad8.data(), cad8, size_t(nc) * 4, hipMemcpyDeviceToHost, s));
            TDX_HIP_CHECK(ctx, hipMemcpyAsync(h_len.data(), clen, size_t(nc) * 4, hipMemcpyDeviceToHost, s));
            TDX_HIP_CHECK(ctx, hipMemcpyAsync(h_recv.data(), crecv, size_t(nc) * 4, hipMemcpyDeviceToHost, s));
            TDX_HIP_CHECK(ctx, hipMemcpyAsync(h_flag.data(), cflag, size_t(nc), hipMemcpyDeviceToHost, s));
        }
        if (stats) stats->launches[TDX_K_MISC] += 4;
    }
    if ((rc = clock.lap(&res->phase_ms[TDX_STREAMNET_COMPACT])) != TDX_OK) return rc;
    if (device_links) {   // ---- links, on the device: label and order are written where the scatter reads them
        streamnet::DeviceColumns DC;
        DC.n = nc; DC.cidx = cidx; DC.p = cp; DC.fel = cfel; DC.ad8 = cad8; DC.len = clen; DC.recv = crecv; DC.flags = cflag;
        std::string why;
        rc = streamnet::build_links_device(ctx, DC, outlet_x, outlet_y, outlet_id, nout, nx, ny, dxA, dyA, gt, clabel, corder, res->links, res->dstats, why);
        if (rc != TDX_OK) return why.empty() ? rc : tdx_fail(ctx, rc, "tdx_streamnet_gpu_links: " + why);
        res->device_built = true;
        res->stream_cells = nc;
        info = static_cast<uint32_t*>(ctx->scratch(TDX_S_A, n * 4));   // (the builder's workspace took the slot)
        if (!info) return TDX_ERR_NOMEM;
    } else {   // ---- links, on the host
        std::vector<int64_t> idx(h_idx.begin(), h_idx.end());
        std::vector<int32_t> outlet(nc, streamnet::LINK_NONE);
        for (int64_t o = 0; o < nout; o++) {   // :514-521: outlets off the raster are dropped, the last one on a cell wins; off the stream they change nothing
            if (outlet_x[o] < 0 || outlet_x[o] >= nx || outlet_y[o] < 0 || outlet_y[o] >= ny) continue;
            const int64_t c = int64_t(outlet_y[o]) * nx + outlet_x[o];
            const auto it = std::lower_bound(idx.begin(), idx.end(), c);
            if (it != idx.end() && *it == c) outlet[size_t(it - idx.begin())] = outlet_id ? outlet_id[o] : int32_t(o + 1);
        }
        streamnet::Compact C;
        C.n = nc; C.idx = idx.data(); C.p = h_p.data(); C.fel = h_fel.data(); C.ad8 = h_ad8.data(); C.len = h_len.data(); C.outlet = outlet.data();
        C.recv = h_recv.data(); C.flags = h_flag.data();
        streamnet::build_links(C, nx, dxA, dyA, gt, res->links);
        res->stream_cells = nc;
    }
    if ((rc = clock.lap(&res->phase_ms[TDX_STREAMNET_LINKS])) != TDX_OK) return rc;
    {   // ---- set-up of the label sweep, the stream cells' labels and orders
        TdxSpan sp(ctx, TDX_K_STENCIL);
        TDX_HIP_CHECK(ctx, hipMemsetAsync(d_ord, 0, n * 2, s));   // the order grid is 0 off the stream, nodata cells included (:1461-1468)
        hipLaunchKernelGGL(label_setup_kernel, grid2, dim3(256), 0, s, d_p, d_src, nx, ny, p_nodata, src_nodata, sw, info, d_w);
        if (nc) {
            if (!device_links) {
                TDX_HIP_CHECK(ctx, hipMemcpyAsync(clabel, res->links.label.data(), size_t(nc) * 4, hipMemcpyHostToDevice, s));
                TDX_HIP_CHECK(ctx, hipMemcpyAsync(corder, res->links.order.data(), size_t(nc) * 2, hipMemcpyHostToDevice, s));
            }
            hipLaunchKernelGGL(scatter_kernel, dim3(tdx_blocks_for(nc, 256)), dim3(256), 0, s, cidx, nc, clabel, corder, sw, d_w, d_ord);
        }
        if (stats) stats->launches[TDX_K_STENCIL] += 2;
    }
    if ((rc = clock.lap(&res->phase_ms[TDX_STREAMNET_SCATTER])) != TDX_OK) return rc;
    {   // ---- watershed labels
        TdxSpan sp(ctx, TDX_K_ACCUM);
        d8sweep::Arrays<d8rev::GageAlg> A{d_w, nullptr, nullptr, nullptr, info};
        int64_t launches_label = 0;   // (the sweeps' counters are apart: rounds / cells_evaluated of the stats are the two sums)
        rc = d8sweep::run(ctx, st, d8rev::GageAlg{}, A, counts, &rounds_label, &launches_label, &outer_label);
        if (rc != TDX_OK) return rc;
        hipLaunchKernelGGL(label_finish_kernel, dim3(tdx_blocks_for(n, 256)), dim3(256), 0, s, d_p, d_src, n, p_nodata, src_nodata, sw, d_w);
        if (stats) stats->launches[TDX_K_ACCUM] += launches_label + 1;
    }
    if ((rc = clock.lap(&res->phase_ms[TDX_STREAMNET_LABEL])) != TDX_OK) return rc;
    TDX_HIP_CHECK(ctx, hipGetLastError());
    res->phase_ms[TDX_STREAMNET_TOTAL] = 0.;
    for (int i = 0; i < TDX_STREAMNET_TOTAL; i++) res->phase_ms[TDX_STREAMNET_TOTAL] += res->phase_ms[i];
    tdx_stats* stt = stats;
    ctx->end_call();
    if (stt) { stt->rounds = outer + outer_label; stt->cells_evaluated = rounds + rounds_label; }
    return TDX_OK;
}

// ---- row strips.  A strip runs the two sweeps on its array (the engine exchanges the record halos) and compacts its OWNED rows; the caller puts the
// strips' compact cells together in strip order (tdx_streamnet_links_build), which is the row-major order of the whole raster, and hands every
// strip its part of the labels and orders back.  A receiver across a cut is found through the rank grid's halo rows: they are exchanged like any
// raster, so they hold the receiver's rank among the NEIGHBOURING strip's stream cells.
int strip_compact_impl(tdx_context* ctx, const Strip& st, int16_t* d_p, int32_t* d_src, const float* d_fel, const float* d_ad8, int64_t row0, int16_t p_nodata,
                       int32_t src_nodata, const double* dxc, const double* dyc, tdx_streamnet_compact* res, tdx_stats* stats) {
    TDX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int nx = st.nx, ny = st.ny_arr;
    const size_t n = size_t(nx) * size_t(ny), first = size_t(st.y0) * size_t(nx), nown = size_t(st.y1 - st.y0) * size_t(nx);
    const unsigned nblocks = tdx_blocks_for(nown, BLOCK_CELLS);
    uint32_t* info = static_cast<uint32_t*>(ctx->scratch(TDX_S_A, n * 4));
    double* step = static_cast<double*>(ctx->scratch(TDX_S_B, n * 8));
    float* len = static_cast<float*>(ctx->scratch(TDX_S_C, n * 4));
    int32_t* rank = static_cast<int32_t*>(ctx->scratch(TDX_S_D, n * 4));
    double* d_step9 = static_cast<double*>(ctx->scratch(TDX_S_F, size_t(ny) * 9 * 8));
    unsigned long long* counts = static_cast<unsigned long long*>(ctx->scratch(TDX_S_M, size_t(tilek::COUNT_RING) * 16));
    uint32_t* block_off = static_cast<uint32_t*>(ctx->scratch(TDX_S_I, size_t(nblocks) * 4 + 16));
    if (!info || !step || !len || !rank || !d_step9 || !counts || !block_off) return TDX_ERR_NOMEM;
    unsigned long long* d_total = reinterpret_cast<unsigned long long*>(block_off + ((size_t(nblocks) + 1) & ~size_t(1)));
    std::vector<double> step9(size_t(ny) * 9, 0.);
    for (int j = 0; j < ny; j++)
        for (int k = 1; k <= 8; k++)
            step9[size_t(j) * 9 + size_t(k)] = (k == 1 || k == 5) ? dxc[j] : (k == 3 || k == 7) ? dyc[j] : sqrt(dxc[j] * dxc[j] + dyc[j] * dyc[j]);
    ctx->begin_call(stats);
    strip_mark(ctx, st, "streamnet: lengths");
    int rc = strip_exchange<int16_t>(ctx, st, d_p, p_nodata);   // p->share(), src->share() (:544-545)
    if (rc != TDX_OK) return rc;
    rc = strip_exchange<int32_t>(ctx, st, d_src, src_nodata);
    if (rc != TDX_OK) return rc;
    int64_t rounds = 0, launches = 0, outer = 1;
    {
        TdxSpan sp(ctx, TDX_K_STENCIL);
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(d_step9, step9.data(), step9.size() * 8, hipMemcpyHostToDevice, s));
        TDX_HIP_CHECK(ctx, hipStreamSynchronize(s));   // `step9` is a local
        hipLaunchKernelGGL(len_setup_kernel, dim3((nx + 63) / 64, (ny + 3) / 4), dim3(256), 0, s, d_p, d_src, nx, ny, p_nodata, src_nodata, d_step9, info, step);
        hipLaunchKernelGGL(d8sweep::init_kernel, dim3(tdx_blocks_for(nown, 256)), dim3(256), 0, s, info, len, first, nown, TDX_ANG_NODATA);
        if (stats) stats->launches[TDX_K_STENCIL] += 2;
    }
    rc = strip_exchange<float>(ctx, st, len, TDX_ANG_NODATA);
    if (rc != TDX_OK) return rc;
    {
        TdxSpan sp(ctx, TDX_K_ACCUM);
        d8sweep::Arrays<StreamLenAlg> A{len, step, nullptr, nullptr, info};
        rc = d8sweep::run(ctx, st, StreamLenAlg{}, A, counts, &rounds, &launches, &outer);
        if (rc != TDX_OK) return rc;
        hipLaunchKernelGGL(d8sweep::finish_kernel, dim3(tdx_blocks_for(nown, 256)), dim3(256), 0, s, len, first, nown, TDX_ANG_NODATA);
        if (stats) stats->launches[TDX_K_ACCUM] += launches + 1;
    }
    uint64_t nc64 = 0;
    {
        TdxSpan sp(ctx, TDX_K_MISC);
        hipLaunchKernelGGL(count_kernel, dim3(nblocks), dim3(256), 0, s, d_p + first, d_src + first, nown, p_nodata, src_nodata, block_off);
        hipLaunchKernelGGL(offsets_kernel, dim3(1), dim3(256), 0, s, block_off, nblocks, d_total);
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(ctx->h_mail + TDX_MAIL_STAGE, d_total, 8, hipMemcpyDeviceToHost, s));
        if ((rc = strip_wait(ctx, st, "the stream cell count")) != TDX_OK) return rc;
        nc64 = ctx->h_mail[TDX_MAIL_STAGE];
    }
    const unsigned nc = unsigned(nc64);
    const size_t ncp = (size_t(nc) + 3) & ~size_t(3);
    uint8_t* buf = static_cast<uint8_t*>(ctx->scratch(TDX_S_H, ncp * (6 * 4 + 2 * 2 + 1) + 64));
    if (!buf) return tdx_fail(ctx, TDX_ERR_NOMEM, "tdx_streamnet_compact_strip: out of device memory");
    uint32_t* cidx = reinterpret_cast<uint32_t*>(buf);
    float* cfel = reinterpret_cast<float*>(buf + ncp * 4);
    float* cad8 = reinterpret_cast<float*>(buf + ncp * 8);
    float* clen = reinterpret_cast<float*>(buf + ncp * 12);
    int32_t* crecv = reinterpret_cast<int32_t*>(buf + ncp * 16);
    int16_t* cp = reinterpret_cast<int16_t*>(buf + ncp * 24);
    uint8_t* cflag = buf + ncp * 28;
    res->nx = nx; res->row_shift = row0 - st.y0;
    res->cidx.resize(nc); res->p.resize(nc); res->fel.resize(nc); res->ad8.resize(nc); res->len.resize(nc); res->recv.resize(nc); res->recv_strip.assign(nc, 0);
    res->flags.resize(nc);
    {
        TdxSpan sp(ctx, TDX_K_MISC);
        TDX_HIP_CHECK(ctx, hipMemsetAsync(rank, 0xff, n * 4, s));   // -1: the halo rows of a strip without a neighbour stay so
        hipLaunchKernelGGL(rank_kernel, dim3(nblocks), dim3(256), 0, s, d_p + first, d_src + first, nown, p_nodata, src_nodata, block_off, rank + first, cidx, uint32_t(first));
    }
    rc = strip_exchange<int32_t>(ctx, st, rank, int32_t(-1));
    if (rc != TDX_OK) return rc;
    if (nc) {
        TdxSpan sp(ctx, TDX_K_MISC);
        hipLaunchKernelGGL(gather_kernel, dim3(tdx_blocks_for(nc, 256)), dim3(256), 0, s, cidx, nc, d_p, d_src, d_fel, d_ad8, len, rank, nx, ny, src_nodata, cp, cfel, cad8,
                           clen, crecv, cflag);
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(res->cidx.data(), cidx, size_t(nc) * 4, hipMemcpyDeviceToHost, s));
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(res->p.data(), cp, size_t(nc) * 2, hipMemcpyDeviceToHost, s));
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(res->fel.data(), cfel, size_t(nc) * 4, hipMemcpyDeviceToHost, s));
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(res->ad8.data(), cad8, size_t(nc) * 4, hipMemcpyDeviceToHost, s));
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(res->len.data(), clen, size_t(nc) * 4, hipMemcpyDeviceToHost, s));
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(res->recv.data(), crecv, size_t(nc) * 4, hipMemcpyDeviceToHost, s));
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(res->flags.data(), cflag, size_t(nc), hipMemcpyDeviceToHost, s));
        if (stats) stats->launches[TDX_K_MISC] += 4;
    }
    if ((rc = strip_wait(ctx, st, "the compact stream cells")) != TDX_OK) return rc;
    static const int hd2[9] = {0, 0, -1, -1, -1, 0, 1, 1, 1};
    for (unsigned i = 0; i < nc; i++) {   // which strip owns the receiver: the one above for a cell of the first owned row that drains north, ...
        const int y = int(res->cidx[i] / uint32_t(nx)), k = res->p[i];
        if (k < 1 || k > 8) continue;
        if (y == st.y0 && hd2[k] < 0) res->recv_strip[i] = -1;
        else if (y == st.y1 - 1 && hd2[k] > 0) res->recv_strip[i] = 1;
    }
    TDX_HIP_CHECK(ctx, hipGetLastError());
    tdx_stats* stt = stats;
    ctx->end_call();
    if (stt) { stt->rounds = outer; stt->cells_evaluated = rounds; }
    return TDX_OK;
}

int strip_label_impl(tdx_context* ctx, const Strip& st, const int16_t* d_p, const int32_t* d_src, int16_t p_nodata, int32_t src_nodata, const tdx_streamnet_compact* part,
                     const int32_t* label, const int16_t* order, int sw, int16_t* d_ord, int32_t* d_w, tdx_stats* stats) {
    TDX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int nx = st.nx, ny = st.ny_arr;
    const size_t n = size_t(nx) * size_t(ny), first = size_t(st.y0) * size_t(nx), nown = size_t(st.y1 - st.y0) * size_t(nx);
    const unsigned nc = unsigned(part->cidx.size());
    const size_t ncp = (size_t(nc) + 3) & ~size_t(3);
    uint32_t* info = static_cast<uint32_t*>(ctx->scratch(TDX_S_A, n * 4));
    unsigned long long* counts = static_cast<unsigned long long*>(ctx->scratch(TDX_S_M, size_t(tilek::COUNT_RING) * 16));
    uint8_t* buf = static_cast<uint8_t*>(ctx->scratch(TDX_S_H, ncp * 10 + 64));
    if (!info || !counts || !buf) return TDX_ERR_NOMEM;
    uint32_t* cidx = reinterpret_cast<uint32_t*>(buf);
    int32_t* clabel = reinterpret_cast<int32_t*>(buf + ncp * 4);
    int16_t* corder = reinterpret_cast<int16_t*>(buf + ncp * 8);
    ctx->begin_call(stats);
    strip_mark(ctx, st, "streamnet: labels");
    int64_t rounds = 0, launches = 0, outer = 1;
    int rc;
    {
        TdxSpan sp(ctx, TDX_K_STENCIL);
        TDX_HIP_CHECK(ctx, hipMemsetAsync(d_ord + first, 0, nown * 2, s));
        hipLaunchKernelGGL(label_setup_kernel, dim3((nx + 63) / 64, (ny + 3) / 4), dim3(256), 0, s, d_p, d_src, nx, ny, p_nodata, src_nodata, sw, info, d_w);
        if (nc) {
            TDX_HIP_CHECK(ctx, hipMemcpyAsync(cidx, part->cidx.data(), size_t(nc) * 4, hipMemcpyHostToDevice, s));
            TDX_HIP_CHECK(ctx, hipMemcpyAsync(clabel, label, size_t(nc) * 4, hipMemcpyHostToDevice, s));
            TDX_HIP_CHECK(ctx, hipMemcpyAsync(corder, order, size_t(nc) * 2, hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(scatter_kernel, dim3(tdx_blocks_for(nc, 256)), dim3(256), 0, s, cidx, nc, clabel, corder, sw, d_w, d_ord);
        }
        if (stats) stats->launches[TDX_K_STENCIL] += 2;
    }
    rc = strip_exchange<uint32_t>(ctx, st, reinterpret_cast<uint32_t*>(d_w), uint32_t(GW_NODATA));   // the neighbours' stream labels and pending cells
    if (rc != TDX_OK) return rc;
    {
        TdxSpan sp(ctx, TDX_K_ACCUM);
        d8sweep::Arrays<d8rev::GageAlg> A{d_w, nullptr, nullptr, nullptr, info};
        rc = d8sweep::run(ctx, st, d8rev::GageAlg{}, A, counts, &rounds, &launches, &outer);
        if (rc != TDX_OK) return rc;
        hipLaunchKernelGGL(label_finish_kernel, dim3(tdx_blocks_for(nown, 256)), dim3(256), 0, s, d_p + first, d_src + first, nown, p_nodata, src_nodata, sw, d_w + first);
        if (stats) stats->launches[TDX_K_ACCUM] += launches + 1;
    }
    TDX_HIP_CHECK(ctx, hipGetLastError());
    tdx_stats* stt = stats;
    ctx->end_call();
    if (stt) { stt->rounds = outer; stt->cells_evaluated = rounds; }
    return TDX_OK;
}

int streamnet_check(tdx_context* ctx, const void* p, const void* src, const void* fel, const void* ad8, int64_t nx, int64_t ny, const void* dxc, const void* dyc,
                    const void* gt, const int32_t* outlet_x, const int32_t* outlet_y, int64_t n_outlets, const void* ord, const void* w, tdx_streamnet_links** links,
                    const char* who) {
    if (!ctx || !p || !src || !fel || !ad8 || !dxc || !dyc || !gt || !ord || !w || !links || nx <= 0 || ny <= 0 || n_outlets < 0 ||
        (n_outlets > 0 && (!outlet_x || !outlet_y)))
        return tdx_fail(ctx, TDX_ERR_ARG, who);
    return too_big(nx, ny) ? tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip") : TDX_OK;
}

}  // namespace

namespace {
int streamnet_dev(tdx_context* ctx, const int16_t* d_p, const int32_t* d_src, const float* d_fel, const float* d_ad8, int64_t nx, int64_t ny, int16_t p_nodata,
                  int32_t src_nodata, const double* dxc, const double* dyc, double dxA, double dyA, const double* gt, const int32_t* outlet_x, const int32_t* outlet_y,
                  const int32_t* outlet_id, int64_t n_outlets, int single_watershed, int16_t* d_ord, int32_t* d_w, tdx_streamnet_links** links, tdx_stats* stats,
                  bool device_links, const char* who) {
    if (int rc = streamnet_check(ctx, d_p, d_src, d_fel, d_ad8, nx, ny, dxc, dyc, gt, outlet_x, outlet_y, n_outlets, d_ord, d_w, links, who)) return rc;
    *links = nullptr;
    tdx_streamnet_links* res = new tdx_streamnet_links;
    const int rc = streamnet_impl(ctx, d_p, d_src, d_fel, d_ad8, int(nx), int(ny), p_nodata, src_nodata, dxc, dyc, dxA, dyA, gt, outlet_x, outlet_y, outlet_id, n_outlets,
                                  single_watershed != 0, d_ord, d_w, res, stats, device_links);
    if (rc != TDX_OK) { delete res; return rc; }   // (a call that had begun was aborted where it failed)
    *links = res;
    return TDX_OK;
}
int streamnet_host(tdx_context* ctx, const int16_t* p, const int32_t* src, const float* fel, const float* ad8, int64_t nx, int64_t ny, int16_t p_nodata, int32_t src_nodata,
                   const double* dxc, const double* dyc, double dxA, double dyA, const double* gt, const int32_t* outlet_x, const int32_t* outlet_y,
                   const int32_t* outlet_id, int64_t n_outlets, int single_watershed, int16_t* ord, int32_t* w, tdx_streamnet_links** links, tdx_stats* stats,
                   bool device_links, const char* who) {
    if (int rc = streamnet_check(ctx, p, src, fel, ad8, nx, ny, dxc, dyc, gt, outlet_x, outlet_y, n_outlets, ord, w, links, who)) return rc;
    HostCall h(ctx, nx, ny);
    int16_t* d_p = h.in(TDX_S_IO0, p);
    int32_t* d_s = h.in(TDX_S_IO1, src);
    float* d_f = h.in(TDX_S_IO2, fel);
    float* d_a = h.in(TDX_S_IO3, ad8);
    int32_t* d_w = h.out(TDX_S_IO4, w);
    int16_t* d_o = h.out(TDX_S_E, ord);
    if (h.error) return h.error;
    const int rc = h.finish(streamnet_dev(ctx, d_p, d_s, d_f, d_a, nx, ny, p_nodata, src_nodata, dxc, dyc, dxA, dyA, gt, outlet_x, outlet_y, outlet_id, n_outlets,
                                          single_watershed, d_o, d_w, links, stats, device_links, who));
    if (rc != TDX_OK && *links) { delete *links; *links = nullptr; }
    return rc;
}
}  // namespace

extern "C" int tdx_streamnet_dev(tdx_context* ctx, const int16_t* d_p, const int32_t* d_src, const float* d_fel, const float* d_ad8, int64_t nx, int64_t ny,
    int16_t p_nodata, int32_t src_nodata, const double* dxc, const double* dyc, double dxA, double dyA, const double* gt, const int32_t* outlet_x,
    const int32_t* outlet_y, const int32_t* outlet_id, int64_t n_outlets, int single_watershed, int16_t* d_ord, int32_t* d_w, tdx_streamnet_links** links,
    tdx_stats* stats) {
    return streamnet_dev(ctx, d_p, d_src, d_fel, d_ad8, nx, ny, p_nodata, src_nodata, dxc, dyc, dxA, dyA, gt, outlet_x, outlet_y, outlet_id, n_outlets, single_watershed, d_ord, d_w,
                         links, stats, false, "tdx_streamnet_dev: bad argument");
}
extern "C" int tdx_streamnet(tdx_context* ctx, const int16_t* p, const int32_t* src, const float* fel, const float* ad8, int64_t nx, int64_t ny,
    int16_t p_nodata, int32_t src_nodata, const double* dxc, const double* dyc, double dxA, double dyA, const double* gt, const int32_t* outlet_x,
    const int32_t* outlet_y, const int32_t* outlet_id, int64_t n_outlets, int single_watershed, int16_t* ord, int32_t* w, tdx_streamnet_links** links,
    tdx_stats* stats) {
    return streamnet_host(ctx, p, src, fel, ad8, nx, ny, p_nodata, src_nodata, dxc, dyc, dxA, dyA, gt, outlet_x, outlet_y, outlet_id, n_outlets, single_watershed, ord, w, links,
                          stats, false, "tdx_streamnet: bad argument");
}
// the same calls with the links built on the device (streamnet_links_device.hip)
extern "C" int tdx_streamnet_gpu_links_dev(tdx_context* ctx, const int16_t* d_p, const int32_t* d_src, const float* d_fel, const float* d_ad8, int64_t nx, int64_t ny,
    int16_t p_nodata, int32_t src_nodata, const double* dxc, const double* dyc, double dxA, double dyA, const double* gt, const int32_t* outlet_x,
    const int32_t* outlet_y, const int32_t* outlet_id, int64_t n_outlets, int single_watershed, int16_t* d_ord, int32_t* d_w, tdx_streamnet_links** links,
    tdx_stats* stats) {
    return streamnet_dev(ctx, d_p, d_src, d_fel, d_ad8, nx, ny, p_nodata, src_nodata, dxc, dyc, dxA, dyA, gt, outlet_x, outlet_y, outlet_id, n_outlets, single_watershed, d_ord, d_w,
                         links, stats, true, "tdx_streamnet_gpu_links_dev: bad argument");
}
extern "C" int tdx_streamnet_gpu_links(tdx_context* ctx, const int16_t* p, const int32_t* src, const float* fel, const float* ad8, int64_t nx, int64_t ny,
    int16_t p_nodata, int32_t src_nodata, const double* dxc, const double* dyc, double dxA, double dyA, const double* gt, const int32_t* outlet_x,
    const int32_t* outlet_y, const int32_t* outlet_id, int64_t n_outlets, int single_watershed, int16_t* ord, int32_t* w, tdx_streamnet_links** links,
    tdx_stats* stats) {
    return streamnet_host(ctx, p, src, fel, ad8, nx, ny, p_nodata, src_nodata, dxc, dyc, dxA, dyA, gt, outlet_x, outlet_y, outlet_id, n_outlets, single_watershed, ord, w, links,
                          stats, true, "tdx_streamnet_gpu_links: bad argument");
}
extern "C" int tdx_streamnet_links_device_phases(const tdx_streamnet_links* links, double* ms, int64_t* jump_rounds, int64_t* level_rounds, int64_t* workspace_bytes) {
    if (!links || !links->device_built) return 0;
    static_assert(int(streamnet::DLINK_PHASES) == TDX_STREAMNET_DLINK_PHASES, "the header's count of sub-phases");
    if (ms) memcpy(ms, links->dstats.ms, sizeof links->dstats.ms);
    if (jump_rounds) *jump_rounds = links->dstats.jump_rounds;
    if (level_rounds) *level_rounds = links->dstats.level_rounds;
    if (workspace_bytes) *workspace_bytes = links->dstats.workspace_bytes;
    return 1;
}

extern "C" int64_t tdx_streamnet_links_count(const tdx_streamnet_links* links, int64_t* n_points, int64_t* stream_cells) {
    if (!links) return 0;
    if (n_points) *n_points = int64_t(links->links.coord.size() / 5);
    if (stream_cells) *stream_cells = links->stream_cells;
    return int64_t(links->links.tree.size() / 9);
}
extern "C" void tdx_streamnet_links_copy(const tdx_streamnet_links* links, int64_t* tree, double* coord, double* phase_ms) {
    if (!links) return;
    if (tree && !links->links.tree.empty()) memcpy(tree, links->links.tree.data(), links->links.tree.size() * sizeof(int64_t));
    if (coord && !links->links.coord.empty()) memcpy(coord, links->links.coord.data(), links->links.coord.size() * sizeof(double));
    if (phase_ms) memcpy(phase_ms, links->phase_ms, sizeof links->phase_ms);
}
extern "C" void tdx_streamnet_links_free(tdx_streamnet_links* links) { delete links; }
extern "C" int tdx_streamnet_write_text(const tdx_streamnet_links* links, const char* treefile, const char* coordfile) {
    if (!links || (!treefile && !coordfile)) return TDX_ERR_ARG;
    auto finish = [](FILE* f) { const bool bad = ferror(f) != 0; return (fclose(f) != 0 || bad) ? TDX_ERR_FILE : TDX_OK; };
    if (treefile) {   // src/streamnet.cpp:1165
        FILE* ft = fopen(treefile, "w");
        if (!ft) return TDX_ERR_FILE;
        const std::vector<int64_t>& t = links->links.tree;
        for (size_t i = 0; i + 9 <= t.size(); i += 9)
            fprintf(ft, "\t%ld\t%ld\t%ld\t%ld\t%ld\t%ld\t%ld\t%ld\t%ld\n", long(t[i]), long(t[i + 1]), long(t[i + 2]), long(t[i + 3]), long(t[i + 4]), long(t[i + 5]),
                    long(t[i + 6]), long(t[i + 7]), long(t[i + 8]));
        if (int rc = finish(ft)) return rc;
    }
    if (coordfile) {   // :1177
        FILE* fc = fopen(coordfile, "w");
        if (!fc) return TDX_ERR_FILE;
        const std::vector<double>& c = links->links.coord;
        for (size_t i = 0; i + 5 <= c.size(); i += 5) fprintf(fc, "\t%f\t%f\t%f\t%f\t%f\n", c[i], c[i + 1], c[i + 2], c[i + 3], c[i + 4]);
        if (int rc = finish(fc)) return rc;
    }
    return TDX_OK;
}

// ---- row strips (see strip_compact_impl)
extern "C" int tdx_streamnet_compact_strip(tdx_context* ctx, const tdx_comm* comm, int16_t* d_p, int32_t* d_src, const float* d_fel, const float* d_ad8, int64_t nx,
                                           int64_t ny_local, int64_t row0, int16_t p_nodata, int32_t src_nodata, const double* dxc, const double* dyc,
                                           tdx_streamnet_compact** part, tdx_stats* stats) {
    if (!ctx || !d_p || !d_src || !d_fel || !d_ad8 || !dxc || !dyc || !part || nx <= 0 || ny_local <= 0 || row0 < 0)
        return tdx_fail(ctx, TDX_ERR_ARG, "tdx_streamnet_compact_strip: bad argument");
    if (too_big(nx, ny_local + 2)) return tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip");
    *part = nullptr;
    tdx_streamnet_compact* res = new tdx_streamnet_compact;
    const int rc = strip_compact_impl(ctx, strip_from_comm(comm, int(nx), int(ny_local)), d_p, d_src, d_fel, d_ad8, row0, p_nodata, src_nodata, dxc, dyc, res, stats);
    if (rc != TDX_OK) { delete res; return rc; }
    *part = res;
    return TDX_OK;
}
extern "C" int64_t tdx_streamnet_compact_count(const tdx_streamnet_compact* part) { return part ? int64_t(part->cidx.size()) : 0; }
extern "C" void tdx_streamnet_compact_free(tdx_streamnet_compact* part) { delete part; }

namespace {
// the parts of all strips put together in strip order: local ranks to global ones
struct MergedParts {
    std::vector<int64_t> idx;
    std::vector<int16_t> p;
    std::vector<float> fel, ad8, len;
    std::vector<int32_t> recv;
    std::vector<uint8_t> flags;
};
int merge_parts(const tdx_streamnet_compact* const* parts, int64_t n_parts, int64_t nx, int64_t ny, const double* gt, const int32_t* outlet_x, const int32_t* outlet_y,
                int64_t n_outlets, tdx_streamnet_links** links, const std::string& who, MergedParts& M) {
    if (!parts || n_parts <= 0 || nx <= 0 || ny <= 0 || !gt || !links || n_outlets < 0 || (n_outlets > 0 && (!outlet_x || !outlet_y)))
        return tdx_fail(nullptr, TDX_ERR_ARG, who + ": bad argument");
    std::vector<int64_t> offset(size_t(n_parts) + 1, 0);
    for (int64_t k = 0; k < n_parts; k++) {
        if (!parts[k] || parts[k]->nx != nx) return tdx_fail(nullptr, TDX_ERR_ARG, who + ": bad argument");
        offset[size_t(k) + 1] = offset[size_t(k)] + int64_t(parts[k]->cidx.size());
    }
    const size_t nc = size_t(offset.back());
    if (nc > 0x7ffffff0ull) return tdx_fail(nullptr, TDX_ERR_ARG, who + ": more than 2^31 stream cells");
    M.idx.resize(nc); M.p.resize(nc); M.fel.resize(nc); M.ad8.resize(nc); M.len.resize(nc); M.recv.resize(nc); M.flags.resize(nc);
    for (int64_t k = 0; k < n_parts; k++) {
        const tdx_streamnet_compact& P = *parts[k];
        for (size_t i = 0, o = size_t(offset[size_t(k)]); i < P.cidx.size(); i++, o++) {
            M.idx[o] = int64_t(P.cidx[i]) + P.row_shift * nx;
            M.p[o] = P.p[i]; M.fel[o] = P.fel[i]; M.ad8[o] = P.ad8[i]; M.len[o] = P.len[i]; M.flags[o] = P.flags[i];
            const int64_t owner = k + P.recv_strip[i];
            M.recv[o] = (P.recv[i] < 0 || owner < 0 || owner >= n_parts) ? -1 : int32_t(offset[size_t(owner)] + P.recv[i]);
        }
    }
    return TDX_OK;
}
}  // namespace

extern "C" int tdx_streamnet_links_build(const tdx_streamnet_compact* const* parts, int64_t n_parts, int64_t nx, int64_t ny, double dxA, double dyA, const double* gt,
                                         const int32_t* outlet_x, const int32_t* outlet_y, const int32_t* outlet_id, int64_t n_outlets, tdx_streamnet_links** links) {
    MergedParts M;
    if (int rc = merge_parts(parts, n_parts, nx, ny, gt, outlet_x, outlet_y, n_outlets, links, "tdx_streamnet_links_build", M)) return rc;
    const size_t nc = M.idx.size();
    std::vector<int32_t> outlet(nc, streamnet::LINK_NONE);
    for (int64_t o = 0; o < n_outlets; o++) {
        if (outlet_x[o] < 0 || outlet_x[o] >= nx || outlet_y[o] < 0 || outlet_y[o] >= ny) continue;
        const int64_t c = int64_t(outlet_y[o]) * nx + outlet_x[o];
        const auto it = std::lower_bound(M.idx.begin(), M.idx.end(), c);
        if (it != M.idx.end() && *it == c) outlet[size_t(it - M.idx.begin())] = outlet_id ? outlet_id[o] : int32_t(o + 1);
    }
    streamnet::Compact C;
    C.n = int64_t(nc); C.idx = M.idx.data(); C.p = M.p.data(); C.fel = M.fel.data(); C.ad8 = M.ad8.data(); C.len = M.len.data(); C.outlet = outlet.data();
    C.recv = M.recv.data(); C.flags = M.flags.data();
    tdx_streamnet_links* res = new tdx_streamnet_links;
    streamnet::build_links(C, nx, dxA, dyA, gt, res->links);
    res->stream_cells = int64_t(nc);
    *links = res;
    return TDX_OK;
}

// The same on the device of ctx: the merged columns are uploaded, the links built there, and label / order come down into the handle with the rows, so
// that tdx_streamnet_label_strip takes the handle unchanged whichever context labels the strip.
extern "C" int tdx_streamnet_links_build_gpu(tdx_context* ctx, const tdx_streamnet_compact* const* parts, int64_t n_parts, int64_t nx, int64_t ny, double dxA, double dyA,
                                             const double* gt, const int32_t* outlet_x, const int32_t* outlet_y, const int32_t* outlet_id, int64_t n_outlets,
                                             tdx_streamnet_links** links) {
    if (!ctx) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_streamnet_links_build_gpu: bad argument");
    MergedParts M;
    if (int rc = merge_parts(parts, n_parts, nx, ny, gt, outlet_x, outlet_y, n_outlets, links, "tdx_streamnet_links_build_gpu", M)) return rc;
    *links = nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    const size_t nc = M.idx.size(), ncp = (nc + 3) & ~size_t(3);
    TDX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    // idx (i64), fel, ad8, len (f32), recv, label (i32), p, order (i16), flags (u8)
    uint8_t* buf = static_cast<uint8_t*>(ctx->scratch(TDX_S_H, ncp * (8 + 5 * 4 + 2 * 2 + 1) + 64));
    if (!buf) return tdx_fail(ctx, TDX_ERR_NOMEM, "tdx_streamnet_links_build_gpu: out of device memory");
    int64_t* d_idx = reinterpret_cast<int64_t*>(buf);
    float* d_fel = reinterpret_cast<float*>(buf + ncp * 8);
    float* d_ad8 = reinterpret_cast<float*>(buf + ncp * 12);
    float* d_len = reinterpret_cast<float*>(buf + ncp * 16);
    int32_t* d_recv = reinterpret_cast<int32_t*>(buf + ncp * 20);
    int32_t* d_label = reinterpret_cast<int32_t*>(buf + ncp * 24);
    int16_t* d_p = reinterpret_cast<int16_t*>(buf + ncp * 28);
    int16_t* d_order = reinterpret_cast<int16_t*>(buf + ncp * 30);
    uint8_t* d_flags = buf + ncp * 32;
    if (nc) {
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(d_idx, M.idx.data(), nc * 8, hipMemcpyHostToDevice, s));
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(d_fel, M.fel.data(), nc * 4, hipMemcpyHostToDevice, s));
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(d_ad8, M.ad8.data(), nc * 4, hipMemcpyHostToDevice, s));
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(d_len, M.len.data(), nc * 4, hipMemcpyHostToDevice, s));
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(d_recv, M.recv.data(), nc * 4, hipMemcpyHostToDevice, s));
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(d_p, M.p.data(), nc * 2, hipMemcpyHostToDevice, s));
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(d_flags, M.flags.data(), nc, hipMemcpyHostToDevice, s));
    }
    tdx_streamnet_links* res = new tdx_streamnet_links;
    streamnet::DeviceColumns DC;
    DC.n = int64_t(nc); DC.idx64 = d_idx; DC.p = d_p; DC.fel = d_fel; DC.ad8 = d_ad8; DC.len = d_len; DC.recv = d_recv; DC.flags = d_flags;
    std::string why;
    int rc = streamnet::build_links_device(ctx, DC, outlet_x, outlet_y, outlet_id, n_outlets, nx, ny, dxA, dyA, gt, d_label, d_order, res->links, res->dstats, why);
    if (rc == TDX_OK) {
        res->links.label.resize(nc);
        res->links.order.resize(nc);
        if (nc) {
            const hipError_t e1 = hipMemcpyAsync(res->links.label.data(), d_label, nc * 4, hipMemcpyDeviceToHost, s);
            const hipError_t e2 = hipMemcpyAsync(res->links.order.data(), d_order, nc * 2, hipMemcpyDeviceToHost, s);
            const hipError_t e3 = hipStreamSynchronize(s);
            if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) { rc = TDX_ERR_HIP; why = "the labels did not come down"; }
        }
    }
    if (rc != TDX_OK) { delete res; return why.empty() ? rc : tdx_fail(ctx, rc, "tdx_streamnet_links_build_gpu: " + why); }
    res->device_built = true;
    res->stream_cells = int64_t(nc);
    res->phase_ms[TDX_STREAMNET_LINKS] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *links = res;
    return TDX_OK;
}

extern "C" int tdx_streamnet_label_strip(tdx_context* ctx, const tdx_comm* comm, const int16_t* d_p, const int32_t* d_src, int64_t nx, int64_t ny_local, int16_t p_nodata,
                                         int32_t src_nodata, const tdx_streamnet_compact* part, const tdx_streamnet_links* links, int64_t first_cell,
                                         int single_watershed, int16_t* d_ord, int32_t* d_w, tdx_stats* stats) {
    if (!ctx || !d_p || !d_src || !part || !links || !d_ord || !d_w || nx <= 0 || ny_local <= 0 || part->nx != nx || first_cell < 0 ||
        size_t(first_cell) + part->cidx.size() > links->links.label.size())
        return tdx_fail(ctx, TDX_ERR_ARG, "tdx_streamnet_label_strip: bad argument");
    if (too_big(nx, ny_local + 2)) return tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip");
    return strip_label_impl(ctx, strip_from_comm(comm, int(nx), int(ny_local)), d_p, d_src, p_nodata, src_nodata, part, links->links.label.data() + first_cell,
                            links->links.order.data() + first_cell, single_watershed != 0, d_ord, d_w, stats);
}
