// The ring builder of the watershed polygons on gfx950: closes, classifies and orders the rings from the edge columns that polygonize.hip leaves in
// device memory (key ascending, successor key, id) and downloads only the finished layer.  The contract is include/taudem_amd_polygonize.h; the host
// builder polygon_rings.cpp is the default and the witness: both make the same arrays of the same edges.
//
// Every edge index is 32-bit (E < 2^32).  No kernel waits for another workgroup; every loop is bounded by E, ny or a round count the host fixes;
// rounds are separate launches, and one "something changed" word per round is read back every second round to stop early.  No atomic decides an
// order: the atomics are integer OR / add / min whose result does not depend on arrival, so two runs give the same bytes.
//   successor  nxt[e] by binary search of next[e] in key; the host's refusals as flag bits; mark[nxt[e]] = 1 + (the side changes): one writer per slot
//   validate   a slot without a writer: the successors are no permutation.  Nothing below runs on edges that failed.
//   label      pointer jumping on the cyclic permutation.  Per edge 16 bytes (m, j, off, w), one 16-byte gather per round: m the smallest edge index
//              within 2^k steps, j the 2^k-th successor, w the corners within 2^k steps, off the corners before the first place m was seen.  A round
//              that changes no m has every m at its cycle's minimum (the leader); off is then the number of corners from e round to the leader, which
//              is the ring rank the host's walk would give, so that label and list ranking are ONE set of rounds.  At most ceil(log2(E)) + 1 rounds.
//              Leaders scanned in key order number the rings.
//   per ring   corner count, smallest vertex (r, c), signed area (the sum of x dy over the vertical edges): runs of one ring within a wave are
//              reduced in registers, one atomic per run
//   rank       the rotation: the rank of the ring's smallest vertex
//   holes      one wave per hole strides up the column of its start vertex, 64 rows at a time, to the first cell whose top side is an edge; that
//              edge's ring is the hole's parent (the outer ring, or a hole of the same piece above); parents are jumped to the outer ring
//   order      three stable radix sorts (hipCUB) over (id, owner's start, own start); scans give vert_first, ring_first, poly_first, ids, cells
//   scatter    every corner to its slot: (rank - rotation) mod corners, the first vertex repeated at the end
#include <algorithm>
#include <chrono>
#include <cstring>
#include <new>
#include <utility>

#include <hipcub/hipcub.hpp>

#include "context.hpp"
#include "device_common.hpp"
#include "polygon_rings_device.hpp"

namespace {

constexpr int TPB = 256;
constexpr uint32_t NONE = 0xffffffffu;
enum : uint32_t { BAD_RANGE = 1, BAD_ORDER = 2, BAD_MISSING = 4, BAD_JOIN = 8, BAD_ID = 16, BAD_PERM = 32, BAD_SHORT = 64, BAD_AREA = 128, BAD_OWNER = 256 };
// the words the host reads back (uint32 each)
enum { W_FLAGS = 0, W_RINGS = 1, W_HOLES = 2, W_POLYS = 3, W_FEATS = 4, W_VERTS = 6 /* uint64 */, W_LABEL_CHANGED = 8, W_OWNER_CHANGED = 48, W_WORDS = 96 };
constexpr int MAX_ROUNDS = 40;

struct Geo { int64_t nx, ny, key_end; };

// start vertex of the edge with this key (the end vertex is the start of side + 1)
__device__ __forceinline__ void edge_start(int64_t key, int side, int64_t nx, int64_t& vc, int64_t& vr) {
    const int64_t cell = key >> 2;
    const int64_t r = cell / nx, c = cell - r * nx;
    vc = c + ((side == 1 || side == 2) ? 1 : 0);
    vr = r + ((side == 2 || side == 3) ? 1 : 0);
}
__device__ __forceinline__ unsigned long long pack_vertex(int64_t vc, int64_t vr) { return (unsigned long long)(vr) << 32 | (unsigned long long)(uint32_t(vc)); }

// first index in [lo, hi) whose key is not below k (hi when there is none); at most 33 steps
__device__ __forceinline__ uint32_t lower_bound(const int64_t* __restrict__ key, uint32_t lo, uint32_t hi, int64_t k) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (key[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Runs of equal `seg` over consecutive lanes of a wave (all 64 lanes call): v is reduced over each run by op; true on the last lane of a run, which
// then holds the run's value.
template <class T, class Op>
__device__ __forceinline__ bool run_reduce(uint32_t seg, T& v, Op op) {
    const int lane = int(threadIdx.x & 63);
    const uint32_t before = __shfl_up(seg, 1, 64), after = __shfl_down(seg, 1, 64);
    int f = (lane == 0 || before != seg) ? 1 : 0;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T u = __shfl_up(v, off, 64);
        const int fu = __shfl_up(f, off, 64);
        if (lane >= off && !f) { v = op(u, v); f = fu; }
    }
    return lane == 63 || after != seg;
}

// state: x = m, y = j, z = off, w = corners of the window
__global__ __launch_bounds__(TPB) void successor_kernel(const int64_t* __restrict__ key, const int64_t* __restrict__ next, const int32_t* __restrict__ id, uint32_t E,
                                                        Geo g, uint4* __restrict__ state, uint8_t* __restrict__ mark, uint32_t* __restrict__ words) {
    const uint64_t i = uint64_t(blockIdx.x) * TPB + threadIdx.x;
    if (i >= E) return;
    const uint32_t e = uint32_t(i);
    const int64_t k = key[e], nk = next[e];
    uint32_t bad = 0;
    if (k < 0 || k >= g.key_end) bad |= BAD_RANGE;
    if (e > 0 && k <= key[e - 1]) bad |= BAD_ORDER;
    const uint32_t at = lower_bound(key, 0, E, nk);
    uint32_t j = e;
    if (at < E && key[at] == nk) {
        j = at;
        const int side = int(k & 3), nside = int(nk & 3);
        int64_t ec, er, sc, sr;
        edge_start(k, (side + 1) & 3, g.nx, ec, er);
        edge_start(nk, nside, g.nx, sc, sr);
        if (ec != sc || er != sr) bad |= BAD_JOIN;
        if (id[at] != id[e]) bad |= BAD_ID;
        mark[at] = uint8_t(1 + (nside != side));
    } else bad |= BAD_MISSING;
    state[e] = make_uint4(e, j, 0u, 0u);
    if (bad) atomicOr(&words[W_FLAGS], bad);
}

__global__ __launch_bounds__(TPB) void validate_kernel(const uint8_t* __restrict__ mark, uint32_t E, uint4* __restrict__ state, uint32_t* __restrict__ words) {
    const uint64_t i = uint64_t(blockIdx.x) * TPB + threadIdx.x;
    if (i >= E) return;
    const uint8_t mk = mark[i];
    if (mk == 0) atomicOr(&words[W_FLAGS], uint32_t(BAD_PERM));
    state[i].w = mk == 2 ? 1u : 0u;
}

__global__ __launch_bounds__(TPB) void jump_kernel(const uint4* __restrict__ in, uint4* __restrict__ out, uint32_t E, uint32_t* __restrict__ changed) {
    const uint64_t i = uint64_t(blockIdx.x) * TPB + threadIdx.x;
    if (i >= E) return;
    uint4 s = in[i];
    const uint4 t = in[s.y];   // s.y < E: an edge index from the start on
    const bool ch = t.x < s.x;
    if (ch) { s.x = t.x; s.z = s.w + t.z; }
    s.w += t.w;
    s.y = t.y;
    out[i] = s;
    if (ch) *changed = 1u;   // every writer writes the same word
}

__global__ __launch_bounds__(TPB) void leader_kernel(const uint4* __restrict__ state, uint32_t E, uint32_t* __restrict__ lead) {
    const uint64_t i = uint64_t(blockIdx.x) * TPB + threadIdx.x;
    if (i < E) lead[i] = state[i].x == uint32_t(i) ? 1u : 0u;
}

// *out = the sum of n flags from their exclusive scan
__global__ void total_kernel(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ ex, uint32_t n, uint32_t* __restrict__ out) { *out = ex[n - 1] + flag[n - 1]; }

struct RingArrays {
    int32_t* id;
    uint32_t* nv;
    unsigned long long* vmin;   // smallest vertex, packed (r, c)
    long long* area;            // signed area in cells: positive for an outer ring
    uint32_t* rot;
};

__global__ __launch_bounds__(TPB) void ring_init_kernel(const uint32_t* __restrict__ lead, const uint32_t* __restrict__ rid, const int32_t* __restrict__ id, uint32_t E, RingArrays R) {
    const uint64_t i = uint64_t(blockIdx.x) * TPB + threadIdx.x;
    if (i >= E || !lead[i]) return;
    const uint32_t q = rid[i];
    R.id[q] = id[i];
    R.nv[q] = 0;
    R.vmin[q] = ~0ull;
    R.area[q] = 0;
    R.rot[q] = 0;
}

// every lane of every wave runs to the end: run_reduce shuffles over all 64
__global__ __launch_bounds__(TPB) void ring_sum_kernel(const int64_t* __restrict__ key, const uint8_t* __restrict__ mark, const uint4* __restrict__ state,
                                                       const uint32_t* __restrict__ rid, uint32_t E, int64_t nx, uint32_t* __restrict__ ring_of, RingArrays R) {
    const uint64_t i = uint64_t(blockIdx.x) * TPB + threadIdx.x;
    const bool valid = i < E;
    uint32_t q = NONE, cnt = 0;
    unsigned long long vm = ~0ull;
    long long ar = 0;
    if (valid) {
        q = rid[state[i].x];
        ring_of[i] = q;
        const int64_t k = key[i];
        const int side = int(k & 3);
        int64_t vc, vr;
        edge_start(k, side, nx, vc, vr);
        if (mark[i] == 2) { cnt = 1; vm = pack_vertex(vc, vr); }
        ar = side == 1 ? vc : side == 3 ? -vc : 0;   // x dy: a right side runs down at x = c + 1, a left side up at x = c
    }
    const bool last_n = run_reduce(q, cnt, [](uint32_t a, uint32_t b) { return a + b; });
    run_reduce(q, vm, [](unsigned long long a, unsigned long long b) { return a < b ? a : b; });
    run_reduce(q, ar, [](long long a, long long b) { return a + b; });
    if (last_n && q != NONE) {
        if (cnt) atomicAdd(&R.nv[q], cnt);
        if (vm != ~0ull) atomicMin(&R.vmin[q], vm);
        if (ar) atomicAdd(reinterpret_cast<unsigned long long*>(&R.area[q]), (unsigned long long)(ar));
    }
}

__global__ __launch_bounds__(TPB) void ring_check_kernel(RingArrays R, uint32_t nr, uint32_t* __restrict__ hole, uint32_t* __restrict__ parent, uint32_t* __restrict__ words) {
    const uint64_t q = uint64_t(blockIdx.x) * TPB + threadIdx.x;
    if (q >= nr) return;
    const long long a = R.area[q];
    uint32_t bad = 0;
    if (R.nv[q] < 4) bad |= BAD_SHORT;
    if (a == 0) bad |= BAD_AREA;
    hole[q] = a < 0 ? 1u : 0u;
    parent[q] = a < 0 ? NONE : uint32_t(q);
    if (bad) atomicOr(&words[W_FLAGS], bad);
}

// the corner at a ring's smallest vertex (a ring passes its smallest vertex once) writes the ring's rotation
__global__ __launch_bounds__(TPB) void rotation_kernel(const int64_t* __restrict__ key, const uint8_t* __restrict__ mark, const uint4* __restrict__ state,
                                                       const uint32_t* __restrict__ ring_of, uint32_t E, int64_t nx, RingArrays R) {
    const uint64_t i = uint64_t(blockIdx.x) * TPB + threadIdx.x;
    if (i >= E || mark[i] != 2) return;
    const uint32_t q = ring_of[i];
    const int64_t k = key[i];
    int64_t vc, vr;
    edge_start(k, int(k & 3), nx, vc, vr);
    if (pack_vertex(vc, vr) != R.vmin[q]) return;
    const uint32_t nv = R.nv[q];   // >= 1: this corner
    R.rot[q] = (nv - state[i].z % nv) % nv;
}

__global__ __launch_bounds__(TPB) void row_first_kernel(const int64_t* __restrict__ key, uint32_t E, Geo g, uint32_t* __restrict__ row_first) {
    const int64_t r = int64_t(blockIdx.x) * TPB + threadIdx.x;
    if (r > g.ny) return;
    row_first[r] = lower_bound(key, 0, E, r * g.nx * 4);
}

__global__ __launch_bounds__(TPB) void compact_kernel(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ ex, uint32_t n, uint32_t* __restrict__ list) {
    const uint64_t q = uint64_t(blockIdx.x) * TPB + threadIdx.x;
    if (q < n && flag[q]) list[ex[q]] = uint32_t(q);
}

// one wave per hole, lane l at row top - l: up the column of the start vertex to the first cell whose top side is an edge
__global__ __launch_bounds__(TPB) void hole_walk_kernel(const int64_t* __restrict__ key, const uint32_t* __restrict__ row_first, const uint32_t* __restrict__ ring_of,
                                                        const uint32_t* __restrict__ holes, uint32_t nholes, Geo g, RingArrays R, uint32_t* __restrict__ parent,
                                                        uint32_t* __restrict__ words) {
    const uint64_t h = (uint64_t(blockIdx.x) * TPB + threadIdx.x) >> 6;   // the same for the 64 lanes of a wave
    const int lane = int(threadIdx.x & 63);
    if (h >= nholes) return;
    const uint32_t q = holes[h];
    const unsigned long long vm = R.vmin[q];
    const int64_t r0 = int64_t(vm >> 32), c0 = int64_t(vm & 0xffffffffull);
    uint32_t found = NONE;
    if (c0 < g.nx && r0 <= g.ny) {
        for (int64_t top = r0 - 1; top >= 0; top -= 64) {   // at most ny / 64 + 1 turns
            const int64_t r = top - lane;
            uint32_t e = NONE;
            if (r >= 0) {
                const int64_t k = (r * g.nx + c0) * 4;
                const uint32_t hi = row_first[r + 1];
                const uint32_t at = lower_bound(key, row_first[r], hi, k);
                if (at < hi && key[at] == k) e = at;
            }
            const unsigned long long b = __ballot(e != NONE);
            if (b) { found = __shfl(e, __ffsll((long long)b) - 1, 64); break; }   // the lowest lane is the nearest row
        }
    }
    if (lane != 0) return;
    uint32_t p = NONE;
    if (found != NONE) {
        const uint32_t Q = ring_of[found];
        if (R.id[Q] == R.id[q]) p = Q;
    }
    if (p == NONE) atomicOr(&words[W_FLAGS], uint32_t(BAD_OWNER));
    else parent[q] = p;
}

__global__ __launch_bounds__(TPB) void owner_jump_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t nr, uint32_t* __restrict__ changed) {
    const uint64_t q = uint64_t(blockIdx.x) * TPB + threadIdx.x;
    if (q >= nr) return;
    const uint32_t p = in[q], pp = in[p];
    out[q] = pp;
    if (pp != p) *changed = 1u;
}

__device__ __forceinline__ unsigned long long vertex_key(unsigned long long packed, int64_t nx) {
    return (packed >> 32) * (unsigned long long)(nx + 1) + (packed & 0xffffffffull);
}

__global__ __launch_bounds__(TPB) void own_key_kernel(RingArrays R, uint32_t nr, int64_t nx, unsigned long long* __restrict__ k, uint32_t* __restrict__ v) {
    const uint64_t q = uint64_t(blockIdx.x) * TPB + threadIdx.x;
    if (q >= nr) return;
    k[q] = vertex_key(R.vmin[q], nx);
    v[q] = uint32_t(q);
}
__global__ __launch_bounds__(TPB) void owner_key_kernel(RingArrays R, const uint32_t* __restrict__ owner, const uint32_t* __restrict__ perm, uint32_t nr, int64_t nx,
                                                        unsigned long long* __restrict__ k) {
    const uint64_t i = uint64_t(blockIdx.x) * TPB + threadIdx.x;
    if (i < nr) k[i] = vertex_key(R.vmin[owner[perm[i]]], nx);
}
__global__ __launch_bounds__(TPB) void id_key_kernel(RingArrays R, const uint32_t* __restrict__ perm, uint32_t nr, uint32_t* __restrict__ k) {
    const uint64_t i = uint64_t(blockIdx.x) * TPB + threadIdx.x;
    if (i < nr) k[i] = uint32_t(R.id[perm[i]]) ^ 0x80000000u;
}

// per place i of the sorted rings: its ring's place, closed vertex count, outer flag, first-of-feature flag
__global__ __launch_bounds__(TPB) void place_kernel(RingArrays R, const uint32_t* __restrict__ order, uint32_t nr, uint32_t* __restrict__ inv,
                                                    unsigned long long* __restrict__ nvc, uint32_t* __restrict__ outer, uint32_t* __restrict__ feat) {
    const uint64_t i = uint64_t(blockIdx.x) * TPB + threadIdx.x;
    if (i >= nr) return;
    const uint32_t q = order[i];
    inv[q] = uint32_t(i);
    nvc[i] = (unsigned long long)(R.nv[q]) + 1;
    const bool o = R.area[q] > 0;
    outer[i] = o ? 1u : 0u;
    feat[i] = (o && (i == 0 || R.id[order[i - 1]] != R.id[q])) ? 1u : 0u;
}

struct Layer {
    int32_t* ids;
    long long* cells;
    long long *poly_first, *ring_first, *vert_first;   // vert_first holds the exclusive scan of the closed vertex counts
};

// every lane runs to the end (run_reduce)
__global__ __launch_bounds__(TPB) void layer_kernel(RingArrays R, const uint32_t* __restrict__ order, uint32_t nr, const uint32_t* __restrict__ outer,
                                                    const uint32_t* __restrict__ feat, const uint32_t* __restrict__ pidx, const uint32_t* __restrict__ fidx, Layer L) {
    const uint64_t i = uint64_t(blockIdx.x) * TPB + threadIdx.x;
    uint32_t f = NONE;
    long long a = 0;
    if (i < nr) {
        const uint32_t q = order[i];
        a = R.area[q];
        f = fidx[i] + feat[i] - 1;   // the first ring of the order is an outer ring and starts feature 0
        if (outer[i]) L.ring_first[pidx[i]] = (long long)(i);
        if (feat[i]) { L.poly_first[fidx[i]] = (long long)(pidx[i]); L.ids[fidx[i]] = R.id[q]; }
    }
    const bool last = run_reduce(f, a, [](long long x, long long y) { return x + y; });
    if (last && f != NONE && a) atomicAdd(reinterpret_cast<unsigned long long*>(&L.cells[f]), (unsigned long long)(a));
}

// the ends of the offset lists and the counts the host reads
__global__ void layer_end_kernel(RingArrays R, const uint32_t* __restrict__ order, uint32_t nr, const uint32_t* __restrict__ outer, const uint32_t* __restrict__ feat,
                                 const uint32_t* __restrict__ pidx, const uint32_t* __restrict__ fidx, Layer L, uint32_t* __restrict__ words) {
    const uint32_t np = pidx[nr - 1] + outer[nr - 1], nf = fidx[nr - 1] + feat[nr - 1];
    const long long nv = L.vert_first[nr - 1] + (long long)(R.nv[order[nr - 1]]) + 1;
    L.ring_first[np] = nr;
    L.poly_first[nf] = np;
    L.vert_first[nr] = nv;
    words[W_POLYS] = np;
    words[W_FEATS] = nf;
    *reinterpret_cast<unsigned long long*>(words + W_VERTS) = (unsigned long long)(nv);
}

__global__ __launch_bounds__(TPB) void scatter_kernel(const int64_t* __restrict__ key, const uint8_t* __restrict__ mark, const uint4* __restrict__ state,
                                                      const uint32_t* __restrict__ ring_of, uint32_t E, int64_t nx, RingArrays R, const uint32_t* __restrict__ inv,
                                                      const long long* __restrict__ vert_first, int2* __restrict__ vert) {
    const uint64_t i = uint64_t(blockIdx.x) * TPB + threadIdx.x;
    if (i >= E || mark[i] != 2) return;
    const uint32_t q = ring_of[i];
    const uint32_t nv = R.nv[q];   // >= 4
    const uint32_t rank = (nv - state[i].z % nv) % nv;
    const uint32_t pos = (rank + nv - R.rot[q]) % nv;
    const int64_t k = key[i];
    int64_t vc, vr;
    edge_start(k, int(k & 3), nx, vc, vr);
    const long long base = vert_first[inv[q]];
    const int2 v = make_int2(int(vc), int(vr));
    vert[base + pos] = v;
    if (pos == 0) vert[base + nv] = v;
}

const char* reason(uint32_t flags) {
    if (flags & BAD_RANGE) return "polygon rings: an edge key outside the raster";
    if (flags & BAD_ORDER) return "polygon rings: edge keys do not ascend (parts out of order?)";
    if (flags & BAD_MISSING) return "polygon rings: the successor of an edge is not among the edges (a strip missing, or parts out of order?)";
    if (flags & BAD_JOIN) return "polygon rings: a successor does not start where its edge ends";
    if (flags & BAD_ID) return "polygon rings: the id changes along a ring";
    if (flags & BAD_PERM) return "polygon rings: the successors are not a permutation of the edges";
    if (flags & BAD_SHORT) return "polygon rings: a ring of fewer than four corners";
    if (flags & BAD_AREA) return "polygon rings: a ring without area";
    return "polygon rings: a hole without an outer ring";
}

// byte offsets into one allocation, every array on a 16-byte boundary
struct Bump {
    size_t off = 0;
    size_t take(size_t bytes) { const size_t o = off; off += (bytes + 15) & ~size_t(15); return o; }
};

}  // namespace

namespace polygons {

int build_rings_device(tdx_context* ctx, const int64_t* d_key, const int64_t* d_next, const int32_t* d_id, uint64_t n_edges, int64_t nx, int64_t ny, Polygons& out,
                       DeviceRingStats& rs, std::string& err) {
    out = Polygons();
    rs = DeviceRingStats();
    if (nx <= 0 || ny <= 0) { err = "polygon rings: bad argument"; return TDX_ERR_ARG; }
    if (nx > (INT64_MAX / 4) / ny) { err = "polygon rings: raster too large for 64-bit keys"; return TDX_ERR_ARG; }
    if (nx >= 0x7fffffff || ny >= 0x7fffffff) { err = "polygon rings: the device builder takes rasters of fewer than 2^31 - 1 columns and rows"; return TDX_ERR_ARG; }
    if (n_edges >= 0xffffffffull) { err = "polygon rings: the device builder takes fewer than 2^32 - 1 edges"; return TDX_ERR_ARG; }
    out.poly_first.assign(1, 0);
    out.ring_first.assign(1, 0);
    out.vert_first.assign(1, 0);
    if (n_edges == 0) return TDX_OK;
    TDX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint32_t E = uint32_t(n_edges);
    const Geo g{nx, ny, nx * ny * 4};
    const unsigned eb = tdx_blocks_for(E, TPB);
    auto t_last = std::chrono::steady_clock::now();
    auto lap = [&](int phase) -> int {
        TDX_HIP_CHECK(ctx, hipStreamSynchronize(s));
        const auto now = std::chrono::steady_clock::now();
        rs.ms[phase] += std::chrono::duration<double, std::milli>(now - t_last).count();
        t_last = now;
        return TDX_OK;
    };
    auto read_words = [&](const uint32_t* d, int n) -> int {   // n uint32 words to the stage mailbox (32 eight-byte words)
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(ctx->h_mail + TDX_MAIL_STAGE, d, size_t(n) * 4, hipMemcpyDeviceToHost, s));
        TDX_HIP_CHECK(ctx, hipStreamSynchronize(s));
        return TDX_OK;
    };
    const uint32_t* mail = reinterpret_cast<const uint32_t*>(ctx->h_mail + TDX_MAIL_STAGE);
    auto refuse = [&](uint32_t flags) { err = reason(flags); out = Polygons(); return TDX_ERR_ARG; };
    int rc;
    size_t tmp_max = 0;
    auto temp = [&](size_t bytes) -> void* { tmp_max = std::max(tmp_max, bytes); return ctx->scratch(TDX_S_D, std::max<size_t>(bytes, 16)); };
    auto scan32 = [&](const uint32_t* in, uint32_t* o, uint32_t n) -> int {
        size_t bytes = 0;
        TDX_HIP_CHECK(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in, o, n, s));
        void* t = temp(bytes);
        if (!t) return TDX_ERR_NOMEM;
        TDX_HIP_CHECK(ctx, hipcub::DeviceScan::ExclusiveSum(t, bytes, in, o, n, s));
        return TDX_OK;
    };

    // ---- the edge-sized workspace: two states of 16 bytes per edge, the marks, the words
    const size_t state_bytes = (size_t(E) * 16 + 255) & ~size_t(255);
    uint8_t* sbuf = static_cast<uint8_t*>(ctx->scratch(TDX_S_A, 2 * state_bytes));
    if (!sbuf) return TDX_ERR_NOMEM;
    const size_t mark_bytes = (size_t(E) + 255) & ~size_t(255);
    uint8_t* mbuf = static_cast<uint8_t*>(ctx->scratch(TDX_S_B, mark_bytes + W_WORDS * 4));
    if (!mbuf) return TDX_ERR_NOMEM;
    rs.workspace_bytes = int64_t(2 * state_bytes + mark_bytes + W_WORDS * 4);
    uint4* st_a = reinterpret_cast<uint4*>(sbuf);
    uint4* st_b = reinterpret_cast<uint4*>(sbuf + state_bytes);
    uint8_t* mark = mbuf;
    uint32_t* words = reinterpret_cast<uint32_t*>(mbuf + mark_bytes);
    TDX_HIP_CHECK(ctx, hipMemsetAsync(mbuf, 0, mark_bytes + W_WORDS * 4, s));

    // ---- successor, validate
    hipLaunchKernelGGL(successor_kernel, dim3(eb), dim3(TPB), 0, s, d_key, d_next, d_id, E, g, st_a, mark, words);
    if ((rc = lap(RING_SUCCESSOR)) != TDX_OK) return rc;
    hipLaunchKernelGGL(validate_kernel, dim3(eb), dim3(TPB), 0, s, mark, E, st_a, words);
    if ((rc = read_words(words, 1)) != TDX_OK) return rc;
    if ((rc = lap(RING_VALIDATE)) != TDX_OK) return rc;
    if (mail[W_FLAGS]) return refuse(mail[W_FLAGS]);

    // ---- label: at most ceil(log2(E)) + 1 rounds
    int bound = 1;
    while ((1ull << (bound - 1)) < uint64_t(E)) bound++;
    if (bound > MAX_ROUNDS) bound = MAX_ROUNDS;   // (E < 2^32: bound <= 33)
    uint4 *cur = st_a, *other = st_b;
    for (int k = 0; k < bound; k++) {
        hipLaunchKernelGGL(jump_kernel, dim3(eb), dim3(TPB), 0, s, cur, other, E, words + W_LABEL_CHANGED + k);
        std::swap(cur, other);
        rs.rounds++;
        if ((k & 1) || k == bound - 1) {
            if ((rc = read_words(words + W_LABEL_CHANGED, k + 1)) != TDX_OK) return rc;
            bool still = false;
            for (int i = 0; i <= k; i++) still = still || mail[i] == 0;
            if (still) break;
        }
    }
    // the ring numbers: leaders in key order.  The other state is free from here on: lead, rid, ring_of (4 bytes per edge each)
    uint32_t* lead = reinterpret_cast<uint32_t*>(other);
    uint32_t* rid = lead + ((size_t(E) + 3) & ~size_t(3));
    uint32_t* ring_of = rid + ((size_t(E) + 3) & ~size_t(3));
    hipLaunchKernelGGL(leader_kernel, dim3(eb), dim3(TPB), 0, s, cur, E, lead);
    if ((rc = scan32(lead, rid, E)) != TDX_OK) return rc;
    hipLaunchKernelGGL(total_kernel, dim3(1), dim3(1), 0, s, lead, rid, E, words + W_RINGS);
    if ((rc = read_words(words, 2)) != TDX_OK) return rc;
    const uint32_t nr = mail[W_RINGS];
    if ((rc = lap(RING_LABEL)) != TDX_OK) return rc;
    if (nr == 0 || nr > E) { err = "polygon rings: impossible ring count"; out = Polygons(); return TDX_ERR_HIP; }

    // ---- the ring-sized workspace
    Bump B;
    const size_t n4 = size_t(nr) * 4, n8 = size_t(nr) * 8;
    const size_t o_id = B.take(n4), o_nv = B.take(n4), o_vmin = B.take(n8), o_area = B.take(n8), o_rot = B.take(n4), o_hole = B.take(n4), o_hpos = B.take(n4),
                 o_holes = B.take(n4), o_par_a = B.take(n4), o_par_b = B.take(n4), o_rows = B.take((size_t(ny) + 1) * 4), o_k64a = B.take(n8), o_k64b = B.take(n8),
                 o_k32a = B.take(n4), o_k32b = B.take(n4), o_va = B.take(n4), o_vb = B.take(n4), o_inv = B.take(n4), o_nvc = B.take(n8), o_outer = B.take(n4),
                 o_feat = B.take(n4), o_pidx = B.take(n4), o_fidx = B.take(n4), o_ids = B.take(n4), o_cells = B.take(n8), o_pf = B.take(n8 + 8), o_rf = B.take(n8 + 8),
                 o_vf = B.take(n8 + 8);
    uint8_t* rb = static_cast<uint8_t*>(ctx->scratch(TDX_S_C, B.off));
    if (!rb) { out = Polygons(); return TDX_ERR_NOMEM; }
    rs.workspace_bytes += int64_t(B.off);
    auto u32 = [&](size_t o) { return reinterpret_cast<uint32_t*>(rb + o); };
    auto u64 = [&](size_t o) { return reinterpret_cast<unsigned long long*>(rb + o); };
    auto i64 = [&](size_t o) { return reinterpret_cast<long long*>(rb + o); };
    const RingArrays R{reinterpret_cast<int32_t*>(rb + o_id), u32(o_nv), u64(o_vmin), i64(o_area), u32(o_rot)};
    const unsigned rbk = tdx_blocks_for(nr, TPB);

    // ---- per ring
    hipLaunchKernelGGL(ring_init_kernel, dim3(eb), dim3(TPB), 0, s, lead, rid, d_id, E, R);
    hipLaunchKernelGGL(ring_sum_kernel, dim3(eb), dim3(TPB), 0, s, d_key, mark, cur, rid, E, nx, ring_of, R);
    hipLaunchKernelGGL(ring_check_kernel, dim3(rbk), dim3(TPB), 0, s, R, nr, u32(o_hole), u32(o_par_a), words);
    if ((rc = scan32(u32(o_hole), u32(o_hpos), nr)) != TDX_OK) return rc;
    hipLaunchKernelGGL(total_kernel, dim3(1), dim3(1), 0, s, u32(o_hole), u32(o_hpos), nr, words + W_HOLES);
    if ((rc = read_words(words, 3)) != TDX_OK) return rc;
    if ((rc = lap(RING_PER_RING)) != TDX_OK) return rc;
    if (mail[W_FLAGS]) return refuse(mail[W_FLAGS]);
    const uint32_t nholes = mail[W_HOLES];

    // ---- rank: the rotation
    hipLaunchKernelGGL(rotation_kernel, dim3(eb), dim3(TPB), 0, s, d_key, mark, cur, ring_of, E, nx, R);
    if ((rc = lap(RING_RANK)) != TDX_OK) return rc;

    // ---- holes
    uint32_t *owner = u32(o_par_a), *owner_other = u32(o_par_b);
    if (nholes) {
        hipLaunchKernelGGL(row_first_kernel, dim3(tdx_blocks_for(uint64_t(ny) + 1, TPB)), dim3(TPB), 0, s, d_key, E, g, u32(o_rows));
        hipLaunchKernelGGL(compact_kernel, dim3(rbk), dim3(TPB), 0, s, u32(o_hole), u32(o_hpos), nr, u32(o_holes));
        hipLaunchKernelGGL(hole_walk_kernel, dim3(tdx_blocks_for(uint64_t(nholes) * 64, TPB)), dim3(TPB), 0, s, d_key, u32(o_rows), ring_of, u32(o_holes), nholes, g, R, owner,
                           words);
        if ((rc = read_words(words, 1)) != TDX_OK) return rc;
        if (mail[W_FLAGS]) { lap(RING_HOLES); return refuse(mail[W_FLAGS]); }
        int obound = 1;   // a chain of parents has at most nholes + 1 rings
        while ((1ull << (obound - 1)) < uint64_t(nholes) + 1) obound++;
        if (obound > MAX_ROUNDS) obound = MAX_ROUNDS;
        for (int k = 0; k < obound; k++) {
            hipLaunchKernelGGL(owner_jump_kernel, dim3(rbk), dim3(TPB), 0, s, owner, owner_other, nr, words + W_OWNER_CHANGED + k);
            std::swap(owner, owner_other);
            if ((k & 1) || k == obound - 1) {
                if ((rc = read_words(words + W_OWNER_CHANGED, k + 1)) != TDX_OK) return rc;
                bool still = false;
                for (int i = 0; i <= k; i++) still = still || mail[i] == 0;
                if (still) break;
            }
        }
    }
    if ((rc = lap(RING_HOLES)) != TDX_OK) return rc;

    // ---- order: stable sorts by own start, owner's start, id; the last key is the first of the order
    {
        const unsigned long long vn = (unsigned long long)(nx + 1) * (unsigned long long)(ny + 1);
        int vbits = 1;
        while (vbits < 64 && (vn >> vbits)) vbits++;
        auto sort = [&](auto* kin, auto* kout, const uint32_t* vin, uint32_t* vout, int bits) -> int {
            size_t bytes = 0;
            TDX_HIP_CHECK(ctx, hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, kin, kout, vin, vout, nr, 0, bits, s));
            void* t = temp(bytes);
            if (!t) return TDX_ERR_NOMEM;
            TDX_HIP_CHECK(ctx, hipcub::DeviceRadixSort::SortPairs(t, bytes, kin, kout, vin, vout, nr, 0, bits, s));
            return TDX_OK;
        };
        hipLaunchKernelGGL(own_key_kernel, dim3(rbk), dim3(TPB), 0, s, R, nr, nx, u64(o_k64a), u32(o_va));
        if ((rc = sort(u64(o_k64a), u64(o_k64b), u32(o_va), u32(o_vb), vbits)) != TDX_OK) return rc;
        hipLaunchKernelGGL(owner_key_kernel, dim3(rbk), dim3(TPB), 0, s, R, owner, u32(o_vb), nr, nx, u64(o_k64a));
        if ((rc = sort(u64(o_k64a), u64(o_k64b), u32(o_vb), u32(o_va), vbits)) != TDX_OK) return rc;
        hipLaunchKernelGGL(id_key_kernel, dim3(rbk), dim3(TPB), 0, s, R, u32(o_va), nr, u32(o_k32a));
        if ((rc = sort(u32(o_k32a), u32(o_k32b), u32(o_va), u32(o_vb), 32)) != TDX_OK) return rc;
    }
    const uint32_t* order = u32(o_vb);
    const Layer L{reinterpret_cast<int32_t*>(rb + o_ids), i64(o_cells), i64(o_pf), i64(o_rf), i64(o_vf)};
    hipLaunchKernelGGL(place_kernel, dim3(rbk), dim3(TPB), 0, s, R, order, nr, u32(o_inv), u64(o_nvc), u32(o_outer), u32(o_feat));
    {
        size_t bytes = 0;
        TDX_HIP_CHECK(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, u64(o_nvc), reinterpret_cast<unsigned long long*>(L.vert_first), nr, s));
        void* t = temp(bytes);
        if (!t) return TDX_ERR_NOMEM;
        TDX_HIP_CHECK(ctx, hipcub::DeviceScan::ExclusiveSum(t, bytes, u64(o_nvc), reinterpret_cast<unsigned long long*>(L.vert_first), nr, s));
    }
    if ((rc = scan32(u32(o_outer), u32(o_pidx), nr)) != TDX_OK) return rc;
    if ((rc = scan32(u32(o_feat), u32(o_fidx), nr)) != TDX_OK) return rc;
    TDX_HIP_CHECK(ctx, hipMemsetAsync(L.cells, 0, n8, s));
    hipLaunchKernelGGL(layer_kernel, dim3(rbk), dim3(TPB), 0, s, R, order, nr, u32(o_outer), u32(o_feat), u32(o_pidx), u32(o_fidx), L);
    hipLaunchKernelGGL(layer_end_kernel, dim3(1), dim3(1), 0, s, R, order, nr, u32(o_outer), u32(o_feat), u32(o_pidx), u32(o_fidx), L, words);
    if ((rc = read_words(words, 8)) != TDX_OK) return rc;
    const uint32_t np = mail[W_POLYS], nf = mail[W_FEATS];
    const uint64_t nvert = *reinterpret_cast<const uint64_t*>(mail + W_VERTS);
    if ((rc = lap(RING_ORDER)) != TDX_OK) return rc;
    if (np == 0 || nf == 0 || np > nr || nf > np || nvert > uint64_t(E) + nr) { err = "polygon rings: impossible layer counts"; out = Polygons(); return TDX_ERR_HIP; }

    // ---- scatter
    int2* d_vert = static_cast<int2*>(ctx->scratch(TDX_S_E, size_t(nvert) * 8));
    if (!d_vert) { out = Polygons(); return TDX_ERR_NOMEM; }
    rs.workspace_bytes += int64_t(size_t(nvert) * 8 + tmp_max);
    hipLaunchKernelGGL(scatter_kernel, dim3(eb), dim3(TPB), 0, s, d_key, mark, cur, ring_of, E, nx, R, u32(o_inv), L.vert_first, d_vert);
    if ((rc = lap(RING_SCATTER)) != TDX_OK) return rc;

    // ---- the finished layer to the host
    try {
        out.id.resize(nf); out.cells.resize(nf); out.poly_first.resize(size_t(nf) + 1); out.ring_first.resize(size_t(np) + 1);
        out.vert_first.resize(size_t(nr) + 1); out.vert.resize(size_t(nvert) * 2);
    } catch (const std::bad_alloc&) {
        out = Polygons();
        err = "polygon rings: out of host memory for the layer";
        return TDX_ERR_NOMEM;
    }
    static_assert(sizeof(long long) == sizeof(int64_t), "offset lists");
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(out.id.data(), L.ids, size_t(nf) * 4, hipMemcpyDeviceToHost, s));
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(out.cells.data(), L.cells, size_t(nf) * 8, hipMemcpyDeviceToHost, s));
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(out.poly_first.data(), L.poly_first, (size_t(nf) + 1) * 8, hipMemcpyDeviceToHost, s));
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(out.ring_first.data(), L.ring_first, (size_t(np) + 1) * 8, hipMemcpyDeviceToHost, s));
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(out.vert_first.data(), L.vert_first, (size_t(nr) + 1) * 8, hipMemcpyDeviceToHost, s));
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(out.vert.data(), d_vert, size_t(nvert) * 8, hipMemcpyDeviceToHost, s));
    TDX_HIP_CHECK(ctx, hipStreamSynchronize(s));
    rs.download_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_last).count();
    TDX_HIP_CHECK(ctx, hipGetLastError());
    return TDX_OK;
}

}  // namespace polygons
