// Watershed polygons on gfx950 (the toolbox step "Watershed Grid To Shapefile", pyfiles/WatershedGridToShapefile.py: one RasterToPolygon call in
// the reference).  The definition is in include/taudem_amd_polygonize.h.
//
// The dense work is the boundary of the id grid: two streaming passes over w, CELLS consecutive cells of the row-major order per thread (the compaction
// of streamnet.hip), so that ranks follow the key order.
//   count   the 4-bit side mask of every cell from its 3 x 3 window, the bits of a block summed
//   scan    the block totals to 64-bit offsets, the edge count to the host; the edge columns are allocated then, sized by the count
//   emit    the masks again; at every edge's rank its key, its successor's key (the cell-local right-turn rule on the same window) and its id
// No atomic decides a rank: the same bytes on every run.  The 3 x 3 window of a thread is three runs of CELLS + 2 cells; where the first owned cell lies
// on a 16-byte boundary and nx is a multiple of 4, every run's inner cells are two 16-byte loads, else cell-wide loads.  A cell outside the readable
// rows reads as nodata, which is "not this id" for every id.
// The rings are closed on the host (polygon_rings.cpp): a walk over the edges, a binary search per successor.  That is the default.  The _gpu_rings
// entry points close them on the device instead (polygon_rings_device.hip): the edge columns stay where emit_kernel left them and only the finished layer
// comes down.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <new>
#include <vector>

#include "context.hpp"
#include "device_common.hpp"
#include "polygon_rings.hpp"
#include "polygon_rings_device.hpp"
#include "strips.hpp"
#include "vector_layer.hpp"

struct tdx_polygonize_edges {
    polygons::EdgePart part;
    double phase_ms[TDX_POLYGONIZE_PHASES] = {0, 0, 0, 0, 0};
};
struct tdx_polygons {
    polygons::Polygons P;
    int64_t edges = 0;
    double phase_ms[TDX_POLYGONIZE_PHASES] = {0, 0, 0, 0, 0};
    bool device_rings = false;          // the rings were closed on the device: rs holds its sub-phases
    polygons::DeviceRingStats rs;
};

namespace {

constexpr int CELLS = 8, BLOCK_CELLS = 256 * CELLS;

// The owned cells of a strip (of the whole raster: one strip without halo rows) and what may be read around them
struct Grid {
    const int32_t* w;   // the first owned cell
    int64_t n_own;      // owned cells
    int64_t lo, hi;     // the readable cells as offsets from w: [lo, hi); the owned rows and the halo rows that lie on the raster
    int64_t cell0;      // the first owned cell's index in the whole raster
    int nx;
    int32_t nd;
};

using i32x4 = int32_t __attribute__((ext_vector_type(4)));

// Every load is unconditional, from the nearest readable place, and what was out of range is replaced afterwards: no branch around a load, so that
// all the loads of a thread are in flight together
__device__ __forceinline__ int32_t load_cell(const Grid& g, int64_t j) {
    const int64_t jc = min(max(j, g.lo), g.hi - 1);
    const int32_t v = g.w[jc];
    return jc == j ? v : g.nd;
}

// v[0 .. CELLS + 1] = cells j0 - 1 .. j0 + CELLS.  VEC: j0, lo and hi are multiples of 4 and w + j0 lies on a 16-byte boundary, so that a group of 4 is
// readable as a whole or not at all
template <bool VEC>
__device__ __forceinline__ void load_run(const Grid& g, int64_t j0, int32_t (&v)[CELLS + 2]) {
    v[0] = load_cell(g, j0 - 1);
    v[CELLS + 1] = load_cell(g, j0 + CELLS);
    if constexpr (VEC) {
#pragma unroll
        for (int h = 0; h < CELLS / 4; h++) {
            const int64_t a = j0 + 4 * h;
            const int64_t ac = min(max(a, g.lo), g.hi - 4);   // lo, hi and a are multiples of 4 and hi - lo >= 4: ac is one too, and readable
            const i32x4 q = *reinterpret_cast<const i32x4*>(g.w + ac);
            const bool in = ac == a;
            v[1 + 4 * h] = in ? q[0] : g.nd; v[2 + 4 * h] = in ? q[1] : g.nd; v[3 + 4 * h] = in ? q[2] : g.nd; v[4 + 4 * h] = in ? q[3] : g.nd;
        }
    } else {
#pragma unroll
        for (int k = 0; k < CELLS; k++) v[1 + k] = load_cell(g, j0 + k);
    }
}

// the 3 x 3 window of one cell; what lies off the raster holds nodata
struct Window { int32_t a, n, ne, e, se, s, sw, w, nw; };

// The three runs of a thread: the rows above, of and below its CELLS cells (a thread past the owned cells loads like any other: every address is
// brought into range)
struct Runs { int32_t up[CELLS + 2], mid[CELLS + 2], dn[CELLS + 2]; };
template <bool VEC>
__device__ __forceinline__ void load_runs(const Grid& g, int64_t i0, Runs& R) {
    load_run<VEC>(g, i0 - g.nx, R.up);
    load_run<VEC>(g, i0, R.mid);
    load_run<VEC>(g, i0 + g.nx, R.dn);
}

// The thread's CELLS windows: f(i, window) for every owned cell i = i0 + k that holds an id
template <class F>
__device__ __forceinline__ void for_cells(const Grid& g, int64_t i0, const Runs& R, F f) {
    const int32_t (&up)[CELLS + 2] = R.up, (&mid)[CELLS + 2] = R.mid, (&dn)[CELLS + 2] = R.dn;
    int c = int(uint64_t(i0) % uint64_t(g.nx));
#pragma unroll
    for (int k = 0; k < CELLS; k++) {
        const int64_t i = i0 + k;
        const int32_t a = mid[k + 1];
        if (i < g.n_own && a != g.nd) {
            const bool west = c > 0, east = c < g.nx - 1;   // the neighbouring columns are on the raster (a run crosses row ends)
            Window q;
            q.a = a; q.n = up[k + 1]; q.s = dn[k + 1];
            q.w = west ? mid[k] : g.nd; q.nw = west ? up[k] : g.nd; q.sw = west ? dn[k] : g.nd;
            q.e = east ? mid[k + 2] : g.nd; q.ne = east ? up[k + 2] : g.nd; q.se = east ? dn[k + 2] : g.nd;
            f(i, q);
        }
        if (++c == g.nx) c = 0;
    }
}

// bit s: side s (0 top, 1 right, 2 bottom, 3 left) is a boundary edge
__device__ __forceinline__ unsigned side_mask(const Window& q) {
    return unsigned(q.n != q.a) | unsigned(q.e != q.a) << 1 | unsigned(q.s != q.a) << 2 | unsigned(q.w != q.a) << 3;
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
    const unsigned s0 = s_wave[0], s1 = s_wave[1], s2 = s_wave[2], s3 = s_wave[3];
    *total = s0 + s1 + s2 + s3;
    return (w > 0 ? s0 : 0u) + (w > 1 ? s1 : 0u) + (w > 2 ? s2 : 0u) + (v - c);
}

__device__ __forceinline__ unsigned thread_count(const Grid& g, int64_t i0, const Runs& R) {
    unsigned n = 0;
    for_cells(g, i0, R, [&](int64_t, const Window& q) { n += unsigned(__popc(side_mask(q))); });
    return n;
}

template <bool VEC>
__global__ __launch_bounds__(256) void count_kernel(Grid g, uint32_t* __restrict__ block_count) {
    const int64_t i0 = int64_t(blockIdx.x) * BLOCK_CELLS + int64_t(threadIdx.x) * CELLS;
    Runs R;
    load_runs<VEC>(g, i0, R);
    unsigned total;
    block_scan(thread_count(g, i0, R), &total);
    if (threadIdx.x == 0) block_count[blockIdx.x] = total;   // at most 4 * BLOCK_CELLS
}

// one block: block_count -> exclusive 64-bit offsets, the sum to *total
__global__ __launch_bounds__(256) void offsets_kernel(const uint32_t* __restrict__ block_count, unsigned nblocks, unsigned long long* __restrict__ block_off,
                                                      unsigned long long* __restrict__ total) {
    __shared__ unsigned long long s_carry;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (unsigned b0 = 0; b0 < nblocks; b0 += 256) {
        const unsigned b = b0 + threadIdx.x;
        const unsigned c = b < nblocks ? block_count[b] : 0u;
        unsigned chunk;   // at most 256 * 4 * BLOCK_CELLS = 2^21
        const unsigned ex = block_scan(c, &chunk);
        const unsigned long long carry = s_carry;
        if (b < nblocks) block_off[b] = carry + ex;
        __syncthreads();   // everybody has read s_carry (and block_scan's words)
        if (threadIdx.x == 0) s_carry = carry + chunk;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = s_carry;
}

// The successor of side s of the cell with key4 = 4 * (its index in the raster): F is the cell ahead in the direction of travel, D the neighbour of F on
// the outside of side s.  F != a: the next side of the cell itself; else D != a: the same side of F; else the previous side of D.
__device__ __forceinline__ int64_t successor(const Window& q, int s, int64_t key4, int64_t nx4) {
    const int32_t a = q.a;
    switch (s) {
    case 0: return q.e != a ? key4 + 1 : q.ne != a ? key4 + 4 : key4 + 4 - nx4 + 3;          // east: E, NE
    case 1: return q.s != a ? key4 + 2 : q.se != a ? key4 + nx4 + 1 : key4 + nx4 + 4;        // south: S, SE
    case 2: return q.w != a ? key4 + 3 : q.sw != a ? key4 - 4 + 2 : key4 + nx4 - 4 + 1;      // west: W, SW
    default: return q.n != a ? key4 : q.nw != a ? key4 - nx4 + 3 : key4 - nx4 - 4 + 2;       // north: N, NW
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void emit_kernel(Grid g, const unsigned long long* __restrict__ block_off, unsigned long long n_edges, int64_t* __restrict__ key,
                                                   int64_t* __restrict__ next, int32_t* __restrict__ id) {
    const int64_t i0 = int64_t(blockIdx.x) * BLOCK_CELLS + int64_t(threadIdx.x) * CELLS;
    Runs R;
    load_runs<VEC>(g, i0, R);
    unsigned total;
    unsigned long long r = block_off[blockIdx.x] + block_scan(thread_count(g, i0, R), &total);
    const int64_t nx4 = int64_t(g.nx) * 4;
    for_cells(g, i0, R, [&](int64_t i, const Window& q) {
        const unsigned m = side_mask(q);
        const int64_t key4 = (g.cell0 + i) * 4;
#pragma unroll
        for (int s = 0; s < 4; s++)
            if (((m >> s) & 1u) && r < n_edges) {   // (r < n_edges always: the count is the sum of the same masks)
                key[r] = key4 + s;
                next[r] = successor(q, s, key4, nx4);
                id[r] = q.a;
                r++;
            }
    });
}

struct PhaseClock {
    tdx_context* ctx;
    std::chrono::steady_clock::time_point t;
    explicit PhaseClock(tdx_context* c) : ctx(c), t(std::chrono::steady_clock::now()) {}
    int lap(double* ms) {   // the wall time since the last lap with the stream drained
        TDX_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        const auto now = std::chrono::steady_clock::now();
        *ms = std::chrono::duration<double, std::milli>(now - t).count();
        t = now;
        return TDX_OK;
    }
};

// the edge columns where emit_kernel left them (scratch slot TDX_S_H)
struct DeviceEdges { const int64_t* key = nullptr; const int64_t* next = nullptr; const int32_t* id = nullptr; uint64_t n = 0; };

// d_arr: an array of ny_local rows (halo == 0: the whole raster) or of ny_local + 2 rows (halo == 1: row 1 is the raster's row row0).
// dev == nullptr: the columns are downloaded into res->part and the call is ended.  Else they stay on the device, nothing is allocated on the host for
// them, and the call stays open: the caller goes on with the rings and ends it.
int edges_impl(tdx_context* ctx, const int32_t* d_arr, int64_t nx, int64_t ny_local, int halo, int64_t row0, int64_t ny_total, int32_t nd, tdx_polygonize_edges* res,
               tdx_stats* stats, const char* who, DeviceEdges* dev = nullptr) {
    TDX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    Grid g;
    g.w = d_arr + (halo ? nx : 0);
    g.n_own = nx * ny_local;
    g.lo = (halo && row0 > 0) ? -nx : 0;
    g.hi = g.n_own + ((halo && row0 + ny_local < ny_total) ? nx : 0);
    g.cell0 = row0 * nx;
    g.nx = int(nx);
    g.nd = nd;
    const bool vec = (reinterpret_cast<uintptr_t>(g.w) & 15u) == 0 && (nx & 3) == 0;
    const unsigned nblocks = tdx_blocks_for(uint64_t(g.n_own), BLOCK_CELLS);
    // block counts (u32), block offsets (u64), the total (u64)
    const size_t off_at = (size_t(nblocks) * 4 + 15) & ~size_t(15);
    uint8_t* sbuf = static_cast<uint8_t*>(ctx->scratch(TDX_S_I, off_at + size_t(nblocks) * 8 + 16));
    if (!sbuf) return TDX_ERR_NOMEM;
    uint32_t* block_count = reinterpret_cast<uint32_t*>(sbuf);
    unsigned long long* block_off = reinterpret_cast<unsigned long long*>(sbuf + off_at);
    unsigned long long* d_total = block_off + nblocks;
    ctx->begin_call(stats);
    ctx->stage = who;
    PhaseClock clock(ctx);
    int rc;
    {
        TdxSpan sp(ctx, TDX_K_STENCIL);
        if (vec) hipLaunchKernelGGL(count_kernel<true>, dim3(nblocks), dim3(256), 0, s, g, block_count);
        else hipLaunchKernelGGL(count_kernel<false>, dim3(nblocks), dim3(256), 0, s, g, block_count);
        if (stats) stats->launches[TDX_K_STENCIL] += 1;
    }
    if ((rc = clock.lap(&res->phase_ms[TDX_POLYGONIZE_COUNT])) != TDX_OK) return rc;
    uint64_t ne = 0;
    {
        TdxSpan sp(ctx, TDX_K_MISC);
        hipLaunchKernelGGL(offsets_kernel, dim3(1), dim3(256), 0, s, block_count, nblocks, block_off, d_total);
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(ctx->h_mail + TDX_MAIL_STAGE, d_total, 8, hipMemcpyDeviceToHost, s));
        TDX_HIP_CHECK(ctx, hipStreamSynchronize(s));
        ne = ctx->h_mail[TDX_MAIL_STAGE];
        if (stats) stats->launches[TDX_K_MISC] += 1;
    }
    if (ne > uint64_t(g.n_own) * 4) return tdx_fail(ctx, TDX_ERR_HIP, std::string(who) + ": impossible edge count");
    // ---- the edge columns, sized by the count: key, successor key (int64), id (int32)
    const size_t nep = (size_t(ne) + 3) & ~size_t(3);
    uint8_t* buf = static_cast<uint8_t*>(ctx->scratch(TDX_S_H, nep * 20 + 64));
    if (!buf) { ctx->abort_call(); return TDX_ERR_NOMEM; }
    int64_t* d_key = reinterpret_cast<int64_t*>(buf);
    int64_t* d_next = reinterpret_cast<int64_t*>(buf + nep * 8);
    int32_t* d_id = reinterpret_cast<int32_t*>(buf + nep * 16);
    if (!dev) try {
        res->part.key.resize(size_t(ne)); res->part.next.resize(size_t(ne)); res->part.id.resize(size_t(ne));
    } catch (const std::bad_alloc&) {
        return tdx_fail(ctx, TDX_ERR_NOMEM, std::string(who) + ": out of host memory for the edges");
    }
    if ((rc = clock.lap(&res->phase_ms[TDX_POLYGONIZE_SCAN])) != TDX_OK) return rc;   // (a first call's allocations are in this phase, not in a pass)
    if (ne) {
        TdxSpan sp(ctx, TDX_K_STENCIL);
        if (vec) hipLaunchKernelGGL(emit_kernel<true>, dim3(nblocks), dim3(256), 0, s, g, block_off, (unsigned long long)ne, d_key, d_next, d_id);
        else hipLaunchKernelGGL(emit_kernel<false>, dim3(nblocks), dim3(256), 0, s, g, block_off, (unsigned long long)ne, d_key, d_next, d_id);
        if (stats) stats->launches[TDX_K_STENCIL] += 1;
    }
    if ((rc = clock.lap(&res->phase_ms[TDX_POLYGONIZE_EMIT])) != TDX_OK) return rc;
    if (dev) {
        dev->key = d_key; dev->next = d_next; dev->id = d_id; dev->n = ne;
        TDX_HIP_CHECK(ctx, hipGetLastError());
        return TDX_OK;
    }
    if (ne) {
        TdxSpan sp(ctx, TDX_K_MISC);
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(res->part.key.data(), d_key, size_t(ne) * 8, hipMemcpyDeviceToHost, s));
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(res->part.next.data(), d_next, size_t(ne) * 8, hipMemcpyDeviceToHost, s));
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(res->part.id.data(), d_id, size_t(ne) * 4, hipMemcpyDeviceToHost, s));
    }
    if ((rc = clock.lap(&res->phase_ms[TDX_POLYGONIZE_DOWNLOAD])) != TDX_OK) return rc;
    TDX_HIP_CHECK(ctx, hipGetLastError());
    ctx->end_call();
    return TDX_OK;
}

int rings_impl(const tdx_polygonize_edges* const* parts, int64_t n_parts, int64_t nx, int64_t ny, tdx_polygons** polygons) {
    std::vector<const polygons::EdgePart*> ep(static_cast<size_t>(n_parts));
    tdx_polygons* res = new tdx_polygons;
    for (int64_t k = 0; k < n_parts; k++) {
        ep[size_t(k)] = &parts[k]->part;
        res->edges += int64_t(parts[k]->part.key.size());
        for (int i = 0; i < TDX_POLYGONIZE_PHASES; i++) res->phase_ms[i] = std::max(res->phase_ms[i], parts[k]->phase_ms[i]);
    }
    const auto t0 = std::chrono::steady_clock::now();
    std::string err;
    bool ok = false;
    try {
        ok = polygons::build_rings(ep.data(), ep.size(), nx, ny, res->P, err);
    } catch (const std::bad_alloc&) {
        delete res;
        return tdx_fail(nullptr, TDX_ERR_NOMEM, "tdx_polygonize_rings: out of host memory");
    }
    if (!ok) { delete res; return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_polygonize_rings: " + err); }
    res->phase_ms[TDX_POLYGONIZE_RINGS] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *polygons = res;
    return TDX_OK;
}

// The rings of edge columns in device memory, closed there; the call (begin_call) is open and is ended here
int device_rings_impl(tdx_context* ctx, const DeviceEdges& de, int64_t nx, int64_t ny, const double* edge_phase_ms, tdx_polygons** polygons, const char* who) {
    tdx_polygons* res = new tdx_polygons;
    res->edges = int64_t(de.n);
    res->device_rings = true;
    if (edge_phase_ms)
        for (int i = 0; i < TDX_POLYGONIZE_PHASES; i++) res->phase_ms[i] = edge_phase_ms[i];
    std::string err;
    const int rc = polygons::build_rings_device(ctx, de.key, de.next, de.id, de.n, nx, ny, res->P, res->rs, err);
    if (rc != TDX_OK) {
        delete res;
        if (rc == TDX_ERR_HIP && err.empty()) return rc;   // TDX_HIP_CHECK has said why
        if (rc == TDX_ERR_NOMEM && err.empty()) { ctx->abort_call(); return rc; }   // scratch() has
        return tdx_fail(ctx, rc, std::string(who) + ": " + err);
    }
    res->phase_ms[TDX_POLYGONIZE_DOWNLOAD] = res->rs.download_ms;
    res->phase_ms[TDX_POLYGONIZE_RINGS] = 0;
    for (int i = 0; i < polygons::RING_PHASES; i++) res->phase_ms[TDX_POLYGONIZE_RINGS] += res->rs.ms[i];
    ctx->end_call();
    *polygons = res;
    return TDX_OK;
}

}  // namespace

extern "C" int tdx_polygonize_gpu_rings_dev(tdx_context* ctx, const int32_t* d_w, int64_t nx, int64_t ny, int32_t w_nodata, tdx_polygons** polygons, tdx_stats* stats) {
    if (!ctx || !d_w || !polygons || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_polygonize_gpu_rings_dev: bad argument");
    if (too_big(nx, ny)) return tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip");
    *polygons = nullptr;
    tdx_polygonize_edges part;
    DeviceEdges de;
    const int rc = edges_impl(ctx, d_w, nx, ny, 0, 0, ny, w_nodata, &part, stats, "tdx_polygonize_gpu_rings", &de);
    if (rc != TDX_OK) return rc;
    return device_rings_impl(ctx, de, nx, ny, part.phase_ms, polygons, "tdx_polygonize_gpu_rings");
}

extern "C" int tdx_polygonize_gpu_rings(tdx_context* ctx, const int32_t* w, int64_t nx, int64_t ny, int32_t w_nodata, tdx_polygons** polygons, tdx_stats* stats) {
    if (!ctx || !w || !polygons || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_polygonize_gpu_rings: bad argument");
    if (too_big(nx, ny)) return tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip");
    HostCall h(ctx, nx, ny);
    const int32_t* d_w = h.in(TDX_S_IO0, w);
    if (h.error) return h.error;
    return h.finish(tdx_polygonize_gpu_rings_dev(ctx, d_w, nx, ny, w_nodata, polygons, stats));
}

extern "C" int tdx_polygonize_rings_gpu(tdx_context* ctx, const tdx_polygonize_edges* const* parts, int64_t n_parts, int64_t nx, int64_t ny, tdx_polygons** polygons,
                                        tdx_stats* stats) {
    if (!ctx || !parts || n_parts <= 0 || nx <= 0 || ny <= 0 || !polygons) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_polygonize_rings_gpu: bad argument");
    for (int64_t k = 0; k < n_parts; k++)
        if (!parts[k]) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_polygonize_rings_gpu: bad argument");
    *polygons = nullptr;
    size_t total = 0;
    double ms[TDX_POLYGONIZE_PHASES] = {0, 0, 0, 0, 0};
    for (int64_t k = 0; k < n_parts; k++) {
        total += parts[k]->part.key.size();
        for (int i = 0; i < TDX_POLYGONIZE_PHASES; i++) ms[i] = std::max(ms[i], parts[k]->phase_ms[i]);
    }
    // the parts joined in the edge columns' slot: key, successor key (int64), id (int32)
    TDX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t nep = (total + 3) & ~size_t(3);
    uint8_t* buf = static_cast<uint8_t*>(ctx->scratch(TDX_S_H, nep * 20 + 64));
    if (!buf) return TDX_ERR_NOMEM;
    ctx->begin_call(stats);
    ctx->stage = "tdx_polygonize_rings_gpu";
    size_t at = 0;
    for (int64_t k = 0; k < n_parts; k++) {
        const polygons::EdgePart& p = parts[k]->part;
        const size_t n = p.key.size();
        if (!n) continue;
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(buf + at * 8, p.key.data(), n * 8, hipMemcpyHostToDevice, ctx->stream));
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(buf + nep * 8 + at * 8, p.next.data(), n * 8, hipMemcpyHostToDevice, ctx->stream));
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(buf + nep * 16 + at * 4, p.id.data(), n * 4, hipMemcpyHostToDevice, ctx->stream));
        at += n;
    }
    TDX_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));   // the parts are the caller's: they may go once the call returns
    DeviceEdges de;
    de.key = reinterpret_cast<const int64_t*>(buf);
    de.next = reinterpret_cast<const int64_t*>(buf + nep * 8);
    de.id = reinterpret_cast<const int32_t*>(buf + nep * 16);
    de.n = total;
    return device_rings_impl(ctx, de, nx, ny, ms, polygons, "tdx_polygonize_rings_gpu");
}

extern "C" int tdx_polygons_ring_phases(const tdx_polygons* polygons, double* ms, int64_t* rounds, int64_t* workspace_bytes) {
    const bool dev = polygons && polygons->device_rings;
    if (ms)
        for (int i = 0; i < polygons::RING_PHASES; i++) ms[i] = dev ? polygons->rs.ms[i] : 0.0;
    if (rounds) *rounds = dev ? polygons->rs.rounds : 0;
    if (workspace_bytes) *workspace_bytes = dev ? polygons->rs.workspace_bytes : 0;
    return dev ? 1 : 0;
}

extern "C" int tdx_polygonize_dev(tdx_context* ctx, const int32_t* d_w, int64_t nx, int64_t ny, int32_t w_nodata, tdx_polygons** polygons, tdx_stats* stats) {
    if (!ctx || !d_w || !polygons || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_polygonize_dev: bad argument");
    if (too_big(nx, ny)) return tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip");
    *polygons = nullptr;
    tdx_polygonize_edges part;
    int rc = edges_impl(ctx, d_w, nx, ny, 0, 0, ny, w_nodata, &part, stats, "tdx_polygonize");
    if (rc != TDX_OK) return rc;
    const tdx_polygonize_edges* parts[1] = {&part};
    rc = rings_impl(parts, 1, nx, ny, polygons);
    if (rc != TDX_OK) ctx->err = g_tdx_thread_error;
    return rc;
}

extern "C" int tdx_polygonize(tdx_context* ctx, const int32_t* w, int64_t nx, int64_t ny, int32_t w_nodata, tdx_polygons** polygons, tdx_stats* stats) {
    if (!ctx || !w || !polygons || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_polygonize: bad argument");
    if (too_big(nx, ny)) return tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip");
    HostCall h(ctx, nx, ny);
    const int32_t* d_w = h.in(TDX_S_IO0, w);
    if (h.error) return h.error;
    return h.finish(tdx_polygonize_dev(ctx, d_w, nx, ny, w_nodata, polygons, stats));
}

extern "C" int tdx_polygonize_edges_strip(tdx_context* ctx, const tdx_comm* /*comm*/, const int32_t* d_w, int64_t nx, int64_t ny_local, int64_t row0, int64_t ny_total,
                                          int32_t w_nodata, tdx_polygonize_edges** part, tdx_stats* stats) {
    if (!ctx || !d_w || !part || nx <= 0 || ny_local <= 0 || row0 < 0 || ny_total < row0 + ny_local)
        return tdx_fail(ctx, TDX_ERR_ARG, "tdx_polygonize_edges_strip: bad argument");
    if (too_big(nx, ny_local + 2)) return tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip");
    if (nx > (INT64_MAX / 8) / ny_total) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_polygonize_edges_strip: raster too large for 64-bit keys");
    *part = nullptr;
    tdx_polygonize_edges* res = new tdx_polygonize_edges;
    const int rc = edges_impl(ctx, d_w, nx, ny_local, 1, row0, ny_total, w_nodata, res, stats, "tdx_polygonize_edges_strip");
    if (rc != TDX_OK) { delete res; return rc; }
    *part = res;
    return TDX_OK;
}

extern "C" int tdx_polygonize_edges_create(const int64_t* keys, const int64_t* next_keys, const int32_t* ids, int64_t n, tdx_polygonize_edges** part) {
    if (!part || n < 0 || (n > 0 && (!keys || !next_keys || !ids))) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_polygonize_edges_create: bad argument");
    tdx_polygonize_edges* res = new tdx_polygonize_edges;
    if (n) {
        res->part.key.assign(keys, keys + n);
        res->part.next.assign(next_keys, next_keys + n);
        res->part.id.assign(ids, ids + n);
    }
    *part = res;
    return TDX_OK;
}
extern "C" int64_t tdx_polygonize_edges_count(const tdx_polygonize_edges* part) { return part ? int64_t(part->part.key.size()) : 0; }
extern "C" void tdx_polygonize_edges_copy(const tdx_polygonize_edges* part, int64_t* keys, int64_t* next_keys, int32_t* ids, double* phase_ms) {
    if (!part) return;
    const size_t n = part->part.key.size();
    if (keys && n) memcpy(keys, part->part.key.data(), n * 8);
    if (next_keys && n) memcpy(next_keys, part->part.next.data(), n * 8);
    if (ids && n) memcpy(ids, part->part.id.data(), n * 4);
    if (phase_ms) memcpy(phase_ms, part->phase_ms, sizeof part->phase_ms);
}
extern "C" void tdx_polygonize_edges_free(tdx_polygonize_edges* part) { delete part; }

extern "C" int tdx_polygonize_rings(const tdx_polygonize_edges* const* parts, int64_t n_parts, int64_t nx, int64_t ny, tdx_polygons** polygons) {
    if (!parts || n_parts <= 0 || nx <= 0 || ny <= 0 || !polygons) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_polygonize_rings: bad argument");
    for (int64_t k = 0; k < n_parts; k++)
        if (!parts[k]) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_polygonize_rings: bad argument");
    *polygons = nullptr;
    return rings_impl(parts, n_parts, nx, ny, polygons);
}

extern "C" int64_t tdx_polygons_count(const tdx_polygons* polygons, int64_t* n_polygons, int64_t* n_rings, int64_t* n_vertices, int64_t* n_edges) {
    if (n_polygons) *n_polygons = polygons ? int64_t(polygons->P.n_polygons()) : 0;
    if (n_rings) *n_rings = polygons ? int64_t(polygons->P.n_rings()) : 0;
    if (n_vertices) *n_vertices = polygons ? int64_t(polygons->P.n_vertices()) : 0;
    if (n_edges) *n_edges = polygons ? polygons->edges : 0;
    return polygons ? int64_t(polygons->P.features()) : 0;
}
extern "C" void tdx_polygons_copy(const tdx_polygons* polygons, int32_t* ids, int64_t* cells, int64_t* poly_first, int64_t* ring_first, int64_t* vert_first,
                                  int32_t* vertices, double* phase_ms) {
    if (!polygons) return;
    const polygons::Polygons& P = polygons->P;
    auto put = [](void* dst, const void* src, size_t bytes) { if (dst && bytes) memcpy(dst, src, bytes); };
    put(ids, P.id.data(), P.id.size() * 4);
    put(cells, P.cells.data(), P.cells.size() * 8);
    put(poly_first, P.poly_first.data(), P.poly_first.size() * 8);
    put(ring_first, P.ring_first.data(), P.ring_first.size() * 8);
    put(vert_first, P.vert_first.data(), P.vert_first.size() * 8);
    put(vertices, P.vert.data(), P.vert.size() * 4);
    put(phase_ms, polygons->phase_ms, sizeof polygons->phase_ms);
}
extern "C" void tdx_polygons_free(tdx_polygons* polygons) { delete polygons; }

extern "C" int tdx_polygons_write(const char* path, const tdx_polygons* polygons, const double* gt) {
    if (!path || !polygons || !gt) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_polygons_write: bad argument");
    if (tdx::layer_kind(path) == tdx::LayerKind::None)
        return tdx_fail(nullptr, TDX_ERR_ARG, std::string("tdx_polygons_write: unsupported output ") + path + ": " + tdx::kPolygonLayerKindsMessage);
    const polygons::Polygons& P = polygons->P;
    tdx::PolygonLayer L;
    const size_t kid = L.add_field("gridcode", tdx::FieldType::Integer, 10), kc = L.add_field("cells", tdx::FieldType::Integer, 12);
    L.resize(P.features());
    for (size_t f = 0; f < P.features(); f++) {
        L.set(f, kid, (long long)P.id[f]);
        L.set(f, kc, (long long)P.cells[f]);
        L.polygons[f].resize(size_t(P.poly_first[f + 1] - P.poly_first[f]));
        for (int64_t p = P.poly_first[f]; p < P.poly_first[f + 1]; p++) {
            tdx::PolygonLayer::Polygon& pg = L.polygons[f][size_t(p - P.poly_first[f])];
            pg.resize(size_t(P.ring_first[size_t(p) + 1] - P.ring_first[size_t(p)]));
            for (int64_t q = P.ring_first[size_t(p)]; q < P.ring_first[size_t(p) + 1]; q++) {
                tdx::PolygonLayer::Ring& rg = pg[size_t(q - P.ring_first[size_t(p)])];
                for (int64_t v = P.vert_first[size_t(q)]; v < P.vert_first[size_t(q) + 1]; v++) {
                    rg.x.push_back(gt[0] + double(P.vert[2 * size_t(v)]) * gt[1]);
                    rg.y.push_back(gt[3] + double(P.vert[2 * size_t(v) + 1]) * gt[5]);
                }
            }
        }
    }
    std::string err;
    if (!tdx::write_polygon_layer(path, L, err)) return tdx_fail(nullptr, TDX_ERR_FILE, err);
    return TDX_OK;
}
