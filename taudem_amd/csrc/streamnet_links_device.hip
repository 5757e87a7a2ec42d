// StreamNet's link builder on gfx950: the contract is streamnet_links_device.hpp, the definition streamnet_links.cpp (the host builder: the default and the
// witness).  The host builder numbers the links from one counter in the order a FIFO pops the stream cells.  That order has a closed form - ascending
// (h, root), h the longest upstream path of a cell in cells, root the compact rank of the seed that path starts from - so no queue runs here:
//   outlets    one thread per outlet finds its cell by binary search; the last outlet on a cell wins by an integer atomicMax of its place in the list
//   inflow     inflow[r][(k - 1 + 4) % 8] = u: one writer per slot.  k(c) = the filled slots; a cell STARTS links ("node") where k != 1 or where an
//              outlet that is not terminal sits; every other cell continues the link of its one inflow
//   jump       pointer jumping up the single inflow: the nearest node strictly upstream of every k == 1 cell and the distance to it, 8 bytes of state,
//              two buffers, at most ceil(log2(n)) + 1 rounds; a cell that has found no node by then lies on a cycle of k == 1 cells and gets nothing
//   level      the nodes are compacted; per node and slot the node its inflow's link comes from and the cells in between.  Rounds over the nodes,
//              leaves first: a node is evaluated in the first round after all its sources (stamps of the round that finished a node; a stamp of the
//              running round counts as unfinished, so a round reads only what earlier launches wrote).  The junction rule is the host's: orders in slot
//              order, the two bubble passes as written, the order from the last two, magnitudes summed.  The number of rounds is the number of links
//              on the longest path: as large as the junction count on a comb-shaped network, whatever the raster size.  Nodes on or below a cycle are
//              never ready; the rounds end when one finishes nothing.
//   number     one stable radix sort of the finished nodes by (h, root), an exclusive scan of the links each creates: the link numbers
//   links      per node the links it creates, then per node the links that end on it (their d, one more point, the outlet id on a k == 1 node), then
//              per chain cell its label, order, one more point, its outlet id.  Point counts are integer adds; a link's outlet id is the one furthest
//              down it - the last the host's walk writes - by an integer max over (position, id).  No atomic decides an order.
//   rows       -tree is the links in descending number, beg / end a scan of the counts in that order; every point goes to beg + its position in the link
// No kernel waits for another workgroup; every loop is bounded by 8 slots, by log2(n) or by the node count.  The host launches, reads a few words back
// every couple of rounds and allocates the result.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <new>
#include <utility>

#include <hipcub/hipcub.hpp>

#include "context.hpp"
#include "device_common.hpp"
#include "streamnet_links_device.hpp"

int tdx_sort_pairs_u64(tdx_context* ctx, int scratch_slot, const uint64_t* keys_in, uint64_t* keys_out, const uint32_t* vals_in, uint32_t* vals_out, size_t n,
                       int end_bit);

namespace {

using streamnet::LINK_NONE;
constexpr int TPB = 256;
enum : uint32_t { CF_K = 15, CF_MAND = 16, CF_TERM = 32, CF_NODE = 64 };
// the words the host reads back (uint32 each)
enum { W_NODES = 0, W_DONE = 1, W_LINKS = 2, W_POINTS = 4 /* uint64 */, W_JUMP = 8, W_WORDS = 48 };
constexpr int MAX_JUMP = 33;

struct Cols {
    uint32_t n;
    const uint32_t* cidx;
    const int64_t* idx64;
    const int16_t* p;
    const float *fel, *ad8, *len;
    const int32_t* recv;
    const uint8_t* flags;
};
__device__ __forceinline__ int64_t raster_index(const Cols& C, uint32_t i) { return C.idx64 ? C.idx64[i] : int64_t(C.cidx[i]); }

// src/streamnet.cpp:514-521: outlets off the raster are dropped, the last one on a cell wins, off the stream they change nothing
__global__ __launch_bounds__(TPB) void outlet_kernel(Cols C, const int32_t* __restrict__ ox, const int32_t* __restrict__ oy, uint32_t nout, int64_t nx, int64_t ny,
                                                     int32_t* __restrict__ owin) {
    const uint32_t o = blockIdx.x * TPB + threadIdx.x;
    if (o >= nout) return;
    const int64_t x = ox[o], y = oy[o];
    if (x < 0 || x >= nx || y < 0 || y >= ny) return;
    const int64_t c = y * nx + x;
    uint32_t lo = 0, hi = C.n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (raster_index(C, mid) < c) lo = mid + 1; else hi = mid;
    }
    if (lo < C.n && raster_index(C, lo) == c) atomicMax(&owin[lo], int32_t(o));
}

__global__ __launch_bounds__(TPB) void inflow_kernel(Cols C, int32_t* __restrict__ inflow) {
    const uint32_t u = blockIdx.x * TPB + threadIdx.x;
    if (u >= C.n) return;
    const int32_t r = C.recv[u];
    const int k = C.p[u];
    if (r < 0 || uint32_t(r) >= C.n || uint32_t(r) == u || k < 1 || k > 8) return;
    inflow[size_t(r) * 8 + size_t((k - 1 + 4) % 8)] = int32_t(u);
}

// state: x = the cell the pointer has reached, y = the steps taken
__global__ __launch_bounds__(TPB) void classify_kernel(Cols C, const int32_t* __restrict__ inflow, const int32_t* __restrict__ owin, uint8_t* __restrict__ cf,
                                                       uint32_t* __restrict__ isnode, uint2* __restrict__ state, int32_t* __restrict__ label, int16_t* __restrict__ order) {
    const uint32_t c = blockIdx.x * TPB + threadIdx.x;
    if (c >= C.n) return;
    int k = 0;
    int32_t one = int32_t(c);
#pragma unroll
    for (int m = 0; m < 8; m++) {
        const int32_t u = inflow[size_t(c) * 8 + m];
        if (u >= 0) { k++; one = u; }
    }
    const bool mand = owin[c] >= 0, term = (C.flags[c] & streamnet::CELL_TERMINAL) != 0;
    const bool node = k != 1 || (mand && !term);
    cf[c] = uint8_t(uint32_t(k) | (mand ? CF_MAND : 0u) | (term ? CF_TERM : 0u) | (node ? CF_NODE : 0u));
    isnode[c] = node ? 1u : 0u;
    state[c] = k == 1 ? make_uint2(uint32_t(one), 1u) : make_uint2(c, 0u);
    label[c] = LINK_NONE;
    order[c] = 0;
}

__global__ __launch_bounds__(TPB) void jump_kernel(const uint8_t* __restrict__ cf, const uint2* __restrict__ in, uint2* __restrict__ out, uint32_t n,
                                                   uint32_t* __restrict__ changed) {
    const uint32_t c = blockIdx.x * TPB + threadIdx.x;
    if (c >= n) return;
    uint2 s = in[c];   // s.x < n: a cell from the start on
    if (!(cf[c] & CF_NODE) && !(cf[s.x] & CF_NODE)) {   // (a cell that is no node has one inflow, and so has a state of its own)
        const uint2 t = in[s.x];
        s.x = t.x;
        s.y += t.y;
        *changed = 1u;   // every writer writes the same word
    }
    out[c] = s;
}

// *out = the sum of n flags from their exclusive scan
__global__ void total_kernel(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ ex, uint32_t n, uint32_t* __restrict__ out) { *out = ex[n - 1] + flag[n - 1]; }

struct Nodes {
    int32_t* cell;      // [nn]
    int32_t* src;       // [nn][8] node of the link that arrives through slot m; -1: no inflow; -2: never (a cycle of k == 1 cells)
    uint32_t* dist;     // [nn][8] cells between that node and the inflow cell
    int32_t* stamp;     // the level round that evaluated the node, 0: not yet
    uint32_t* h;
    uint32_t* root;
    int32_t* ord;
    long long* mag;
    uint32_t* perm;     // the slots after the bubble passes, 4 bits each
    uint32_t* cnt;      // links created
    uint32_t* base;     // number of the first of them
};
__device__ __forceinline__ int32_t link_below(const Nodes& N, int32_t s) { return int32_t(N.base[s] + N.cnt[s] - 1); }   // the last link a node creates goes on below it

__global__ __launch_bounds__(TPB) void node_kernel(uint32_t n, const int32_t* __restrict__ inflow, const uint8_t* __restrict__ cf, const uint32_t* __restrict__ nid,
                                                   const uint2* __restrict__ state, Nodes N) {
    const uint32_t c = blockIdx.x * TPB + threadIdx.x;
    if (c >= n || !(cf[c] & CF_NODE)) return;
    const uint32_t e = nid[c];
    N.cell[e] = int32_t(c);
    N.stamp[e] = 0;
#pragma unroll
    for (int m = 0; m < 8; m++) {
        const int32_t u = inflow[size_t(c) * 8 + m];
        int32_t s = -1;
        uint32_t d = 0;
        if (u >= 0) {
            if (cf[u] & CF_NODE) s = int32_t(nid[u]);
            else {
                const uint2 t = state[u];
                if (cf[t.x] & CF_NODE) { s = int32_t(nid[t.x]); d = t.y; } else s = -2;
            }
        }
        N.src[size_t(e) * 8 + m] = s;
        N.dist[size_t(e) * 8 + m] = d;
    }
}

__global__ __launch_bounds__(TPB) void level_kernel(Nodes N, uint32_t nn, const uint8_t* __restrict__ cf, int32_t round, uint32_t* __restrict__ done) {
    const uint32_t e = blockIdx.x * TPB + threadIdx.x;
    if (e >= nn || N.stamp[e] != 0) return;
    uint32_t ent[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // (order << 4) | slot, in slot order
    int k = 0;
    unsigned long long best = 0;
    long long mag = 0;
#pragma unroll
    for (int m = 0; m < 8; m++) {
        const int32_t s = N.src[size_t(e) * 8 + m];
        if (s == -1) continue;
        if (s < 0) return;
        const int32_t st = __atomic_load_n(&N.stamp[s], __ATOMIC_RELAXED);
        if (st == 0 || st >= round) return;   // finished by an earlier launch, or not at all
        const uint32_t v = (uint32_t(N.ord[s]) << 4) | uint32_t(m);
#pragma unroll
        for (int j = 0; j < 8; j++) if (j == k) ent[j] = v;
        k++;
        const unsigned long long key = ((unsigned long long)(N.h[s] + N.dist[size_t(e) * 8 + m]) << 32) | N.root[s];
        best = key > best ? key : best;
        mag += N.mag[s];
    }
    uint32_t o = 1, perm = 0, h = 0, root = uint32_t(N.cell[e]);
    if (k == 0) mag = 1;
    else {
        h = uint32_t(best >> 32) + 1;
        root = uint32_t(best);
#pragma unroll
        for (int a = 0; a < 2; a++)   // src/streamnet.cpp:839-851 exactly as written: two bubble passes, whose tie order decides u1 and u2
#pragma unroll
            for (int b = 0; b < 7; b++)
                if (b + 1 < k && (ent[b] >> 4) > (ent[b + 1] >> 4)) { const uint32_t t = ent[b]; ent[b] = ent[b + 1]; ent[b + 1] = t; }
        uint32_t top = 0, second = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            if (j == k - 1) top = ent[j] >> 4;
            if (j == k - 2) second = ent[j] >> 4;
            perm |= (ent[j] & 15u) << (4 * j);
        }
        o = (k >= 2 && second == top) ? top + 1 : top;
    }
    N.h[e] = h; N.root[e] = root; N.ord[e] = int32_t(o); N.mag[e] = mag; N.perm[e] = perm;
    __atomic_store_n(&N.stamp[e], round, __ATOMIC_RELAXED);
    atomicAdd(done, 1u);
}

__global__ __launch_bounds__(TPB) void count_kernel(Nodes N, uint32_t nn, const uint8_t* __restrict__ cf, unsigned long long* __restrict__ key, uint32_t* __restrict__ val) {
    const uint32_t e = blockIdx.x * TPB + threadIdx.x;
    if (e >= nn) return;
    const uint32_t f = cf[N.cell[e]], k = f & CF_K;
    const bool done = N.stamp[e] != 0, extra = (f & CF_MAND) && !(f & CF_TERM);
    N.cnt[e] = done ? (k == 0 ? 1u : k >= 2 ? k - 1 : 0u) + (extra ? 1u : 0u) : 0u;
    key[e] = done ? ((unsigned long long)(N.h[e]) << 32) | N.root[e] : ~0ull;
    val[e] = e;
}
__global__ __launch_bounds__(TPB) void sorted_count_kernel(Nodes N, uint32_t nn, const uint32_t* __restrict__ val, uint32_t* __restrict__ cs) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i < nn) cs[i] = N.cnt[val[i]];
}
__global__ __launch_bounds__(TPB) void base_kernel(Nodes N, uint32_t nn, const uint32_t* __restrict__ val, const uint32_t* __restrict__ cs, const uint32_t* __restrict__ bs,
                                                   uint32_t* __restrict__ words) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i >= nn) return;
    N.base[val[i]] = bs[i];
    if (i == nn - 1) words[W_LINKS] = bs[i] + cs[i];
}

struct LinkArrays {
    int32_t *u1, *u2, *d, *ord, *first;   // u1, u2, d start at -1
    long long* mag;
    uint32_t *dbl, *cnt;
    unsigned long long* shape;            // (position + 1) << 32 | outlet id, 0: none
    unsigned long long* beg;
};
__device__ __forceinline__ unsigned long long shape_key(uint32_t pos, int32_t id) { return ((unsigned long long)(pos) + 1) << 32 | (unsigned long long)(uint32_t(id)); }
__device__ __forceinline__ int32_t outlet_of(const int32_t* __restrict__ owin, const int32_t* __restrict__ ids, uint32_t c) { return ids ? ids[owin[c]] : owin[c] + 1; }

// the links a node creates (src/linklib.h:436-485 through streamnet_links.cpp), its own label and order
__global__ __launch_bounds__(TPB) void links_init_kernel(Nodes N, uint32_t nn, const uint8_t* __restrict__ cf, const int32_t* __restrict__ owin, const int32_t* __restrict__ ids,
                                                         LinkArrays L, uint32_t nl, int32_t* __restrict__ label, int16_t* __restrict__ order) {
    const uint32_t e = blockIdx.x * TPB + threadIdx.x;
    if (e >= nn || N.stamp[e] == 0) return;
    const uint32_t c = uint32_t(N.cell[e]), f = cf[c];
    const int k = int(f & CF_K);
    const bool mand = f & CF_MAND, term = f & CF_TERM, extra = mand && !term;
    const uint32_t again = (mand || term) ? 1u : 0u;   // append_again on the last link made of the inflows (k != 1)
    const int32_t b = int32_t(N.base[e]), body = k == 0 ? 1 : k >= 2 ? k - 1 : 0, o = N.ord[e];
    if (uint32_t(b) + uint32_t(body) + (extra ? 1u : 0u) > nl) return;   // (cannot happen: nl is the sum of these)
    int32_t last;
    if (k == 0) {
        L.first[b] = int32_t(c); L.ord[b] = 1; L.mag[b] = 1; L.dbl[b] = again; L.cnt[b] = 1 + again;
        last = b;
    } else if (k >= 2) {
        const uint32_t perm = N.perm[e];
        const int32_t s_top = N.src[size_t(e) * 8 + ((perm >> (4 * (k - 1))) & 15u)];
        int32_t u1 = link_below(N, s_top);
        long long mag = N.mag[s_top];
        for (int m = 2; m <= k; m++) {   // the links of a k >= 3 junction are chained: the new link is the next one's u1
            const int32_t s2 = N.src[size_t(e) * 8 + ((perm >> (4 * (k - m))) & 15u)], a = b + m - 2;
            const uint32_t dbl = m < k ? 1u : again;
            mag += N.mag[s2];
            L.u1[a] = u1; L.u2[a] = link_below(N, s2); L.first[a] = int32_t(c); L.ord[a] = o; L.mag[a] = mag; L.dbl[a] = dbl; L.cnt[a] = 1 + dbl;
            if (m < k) L.d[a] = a + 1;
            u1 = a;
        }
        last = b + body - 1;
    } else {
        int32_t s = -1;
#pragma unroll
        for (int m = 0; m < 8; m++) { const int32_t t = N.src[size_t(e) * 8 + m]; if (t >= 0) s = t; }
        last = link_below(N, s);
    }
    if (k != 1 && mand) L.shape[last] = shape_key(0, outlet_of(owin, ids, c));
    label[c] = last;
    order[c] = int16_t(o);
    if (extra) {   // the link ends here with the outlet's id; below it a new link of the same order and magnitude
        const int32_t a = b + body;
        L.u1[a] = last; L.first[a] = int32_t(c); L.ord[a] = o; L.mag[a] = N.mag[e]; L.dbl[a] = 0; L.cnt[a] = 1;
        if (k != 1) L.d[last] = a;
    }
}

// the links that end on a node: the node is one more point of each, and their d
__global__ __launch_bounds__(TPB) void links_end_kernel(Nodes N, uint32_t nn, const uint8_t* __restrict__ cf, const int32_t* __restrict__ owin, const int32_t* __restrict__ ids,
                                                        LinkArrays L, uint32_t nl) {
    const uint32_t e = blockIdx.x * TPB + threadIdx.x;
    if (e >= nn || N.stamp[e] == 0) return;
    const uint32_t c = uint32_t(N.cell[e]);
    const int k = int(cf[c] & CF_K);
    if (k == 0) return;
    const int32_t b = int32_t(N.base[e]);
    const uint32_t perm = N.perm[e];
#pragma unroll
    for (int m = 0; m < 8; m++) {
        const int32_t s = N.src[size_t(e) * 8 + m];
        if (s < 0) continue;
        const int32_t a = link_below(N, s);
        if (uint32_t(a) >= nl) continue;
        atomicAdd(&L.cnt[a], 1u);
        if (k == 1) {
            L.d[a] = b;
            atomicMax(&L.shape[a], shape_key(N.dist[size_t(e) * 8 + m] + 1, outlet_of(owin, ids, c)));
        } else {
            int j = 0;
#pragma unroll
            for (int i = 0; i < 8; i++) if (i < k && ((perm >> (4 * i)) & 15u) == uint32_t(m)) j = i;
            L.d[a] = b + (k - 1 - j > 1 ? k - 1 - j : 1) - 1;
        }
    }
}

// a cell with one inflow that starts no link continues the link below the nearest node upstream
__global__ __launch_bounds__(TPB) void cells_kernel(uint32_t n, const uint8_t* __restrict__ cf, const uint2* __restrict__ state, const uint32_t* __restrict__ nid, Nodes N,
                                                    const int32_t* __restrict__ owin, const int32_t* __restrict__ ids, LinkArrays L, uint32_t nl,
                                                    int32_t* __restrict__ label, int16_t* __restrict__ order) {
    const uint32_t c = blockIdx.x * TPB + threadIdx.x;
    if (c >= n || (cf[c] & CF_NODE)) return;
    const uint2 s = state[c];
    if (!(cf[s.x] & CF_NODE)) return;
    const uint32_t e = nid[s.x];
    if (N.stamp[e] == 0) return;
    const int32_t a = link_below(N, int32_t(e));
    if (uint32_t(a) >= nl) return;
    label[c] = a;
    order[c] = int16_t(N.ord[e]);
    atomicAdd(&L.cnt[a], 1u);
    if (cf[c] & CF_MAND) atomicMax(&L.shape[a], shape_key(s.y, outlet_of(owin, ids, c)));
}

__global__ __launch_bounds__(TPB) void rev_count_kernel(LinkArrays L, uint32_t nl, unsigned long long* __restrict__ cr) {
    const uint32_t t = blockIdx.x * TPB + threadIdx.x;
    if (t < nl) cr[t] = L.cnt[nl - 1 - t];
}
// rows in the order of the reference's list, which inserts at its head: the last link first
__global__ __launch_bounds__(TPB) void tree_kernel(LinkArrays L, uint32_t nl, const unsigned long long* __restrict__ begr, long long* __restrict__ tree,
                                                   uint32_t* __restrict__ words) {
    const uint32_t t = blockIdx.x * TPB + threadIdx.x;
    if (t >= nl) return;
    const uint32_t a = nl - 1 - t;
    const unsigned long long beg = begr[t], sk = L.shape[a];
    const uint32_t cnt = L.cnt[a];
    L.beg[a] = beg;
    long long* row = tree + size_t(t) * 9;
    row[0] = a; row[1] = (long long)(beg); row[2] = (long long)(beg + cnt) - 1; row[3] = L.d[a]; row[4] = L.u1[a]; row[5] = L.u2[a]; row[6] = L.ord[a];
    row[7] = sk ? (long long)(int32_t(uint32_t(sk))) : -1; row[8] = L.mag[a];
    if (t == nl - 1) *reinterpret_cast<unsigned long long*>(words + W_POINTS) = beg + cnt;
}

struct Geo {
    int64_t nx;
    double gt0, gt1, gt2, gt3, cellarea;
    unsigned long long np;
};
// one row of the -coord file; the build's -ffp-contract=off keeps the sums as the host rounds them
__device__ __forceinline__ void put_point(const Cols& C, const Geo& g, double* __restrict__ coord, unsigned long long row, uint32_t c) {
    if (row >= g.np) return;
    const int64_t idx = raster_index(C, c);
    const int64_t x = idx % g.nx, y = idx / g.nx;
    const float area = float(double(C.ad8[c]) * g.cellarea);   // float * double, stored as float (src/linklib.h:836)
    double* pt = coord + size_t(row) * 5;
    pt[0] = g.gt0 + g.gt1 / 2. + double(x) * g.gt1;
    pt[1] = g.gt2 - g.gt3 / 2. - double(y) * g.gt3;
    pt[2] = C.len[c];
    pt[3] = C.fel[c];
    pt[4] = area;
}
__global__ __launch_bounds__(TPB) void coord_first_kernel(Cols C, Geo g, LinkArrays L, uint32_t nl, double* __restrict__ coord) {
    const uint32_t a = blockIdx.x * TPB + threadIdx.x;
    if (a >= nl) return;
    put_point(C, g, coord, L.beg[a], uint32_t(L.first[a]));
    if (L.dbl[a]) put_point(C, g, coord, L.beg[a] + 1, uint32_t(L.first[a]));
}
__global__ __launch_bounds__(TPB) void coord_node_kernel(Cols C, Geo g, Nodes N, uint32_t nn, LinkArrays L, uint32_t nl, double* __restrict__ coord) {
    const uint32_t e = blockIdx.x * TPB + threadIdx.x;
    if (e >= nn || N.stamp[e] == 0) return;
#pragma unroll
    for (int m = 0; m < 8; m++) {
        const int32_t s = N.src[size_t(e) * 8 + m];
        if (s < 0) continue;
        const int32_t a = link_below(N, s);
        if (uint32_t(a) >= nl) continue;
        put_point(C, g, coord, L.beg[a] + N.dist[size_t(e) * 8 + m] + 1 + L.dbl[a], uint32_t(N.cell[e]));
    }
}
__global__ __launch_bounds__(TPB) void coord_cell_kernel(Cols C, Geo g, const uint8_t* __restrict__ cf, const uint2* __restrict__ state, const uint32_t* __restrict__ nid, Nodes N,
                                                         LinkArrays L, uint32_t nl, double* __restrict__ coord) {
    const uint32_t c = blockIdx.x * TPB + threadIdx.x;
    if (c >= C.n || (cf[c] & CF_NODE)) return;
    const uint2 s = state[c];
    if (!(cf[s.x] & CF_NODE)) return;
    const uint32_t e = nid[s.x];
    if (N.stamp[e] == 0) return;
    const int32_t a = link_below(N, int32_t(e));
    if (uint32_t(a) >= nl) return;
    put_point(C, g, coord, L.beg[a] + s.y + L.dbl[a], c);
}

// byte offsets into one allocation, every array on a 16-byte boundary
struct Bump {
    size_t off = 0;
    size_t take(size_t bytes) { const size_t o = off; off += (bytes + 15) & ~size_t(15); return o; }
};

}  // namespace

namespace streamnet {

int build_links_device(tdx_context* ctx, const DeviceColumns& DC, const int32_t* outlet_x, const int32_t* outlet_y, const int32_t* outlet_id, int64_t n_outlets,
                       int64_t nx, int64_t ny, double dxA, double dyA, const double* gt, int32_t* d_label, int16_t* d_order, Links& out, DeviceLinkStats& ds,
                       std::string& err) {
    out = Links();
    ds = DeviceLinkStats();
    if (DC.n < 0 || nx <= 0 || ny <= 0 || !gt || n_outlets < 0 || (n_outlets > 0 && (!outlet_x || !outlet_y))) { err = "streamnet links: bad argument"; return TDX_ERR_ARG; }
    if (DC.n >= 0x7fffffffll) { err = "streamnet links: the device builder takes fewer than 2^31 - 1 stream cells"; return TDX_ERR_ARG; }
    if (n_outlets >= 0x7fffffffll) { err = "streamnet links: the device builder takes fewer than 2^31 - 1 outlets"; return TDX_ERR_ARG; }
    if (DC.n == 0) return TDX_OK;
    if (!DC.p || !DC.fel || !DC.ad8 || !DC.len || !DC.recv || !DC.flags || (!DC.cidx && !DC.idx64) || !d_label || !d_order) { err = "streamnet links: bad argument"; return TDX_ERR_ARG; }
    TDX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint32_t n = uint32_t(DC.n), nout = uint32_t(n_outlets);
    const Cols C{n, DC.cidx, DC.idx64, DC.p, DC.fel, DC.ad8, DC.len, DC.recv, DC.flags};
    const unsigned cb = tdx_blocks_for(n, TPB);
    auto t_last = std::chrono::steady_clock::now();
    auto lap = [&](int phase) -> int {
        TDX_HIP_CHECK(ctx, hipStreamSynchronize(s));
        const auto now = std::chrono::steady_clock::now();
        ds.ms[phase] += std::chrono::duration<double, std::milli>(now - t_last).count();
        t_last = now;
        return TDX_OK;
    };
    auto read_words = [&](const uint32_t* d, int nw) -> int {   // nw uint32 words to the stage mailbox (32 eight-byte words)
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(ctx->h_mail + TDX_MAIL_STAGE, d, size_t(nw) * 4, hipMemcpyDeviceToHost, s));
        TDX_HIP_CHECK(ctx, hipStreamSynchronize(s));
        return TDX_OK;
    };
    const uint32_t* mail = reinterpret_cast<const uint32_t*>(ctx->h_mail + TDX_MAIL_STAGE);
    int rc;
    size_t tmp_max = 0;
    auto temp = [&](size_t bytes) -> void* { tmp_max = std::max(tmp_max, bytes); return ctx->scratch(TDX_S_D, std::max<size_t>(bytes, 16)); };
    auto scan32 = [&](const uint32_t* in, uint32_t* o, uint32_t cnt) -> int {
        size_t bytes = 0;
        TDX_HIP_CHECK(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in, o, cnt, s));
        void* t = temp(bytes);
        if (!t) return TDX_ERR_NOMEM;
        TDX_HIP_CHECK(ctx, hipcub::DeviceScan::ExclusiveSum(t, bytes, in, o, cnt, s));
        return TDX_OK;
    };

    // ---- the cell-sized workspace
    Bump B;
    const size_t o_inflow = B.take(size_t(n) * 32), o_sa = B.take(size_t(n) * 8), o_sb = B.take(size_t(n) * 8), o_owin = B.take(size_t(n) * 4), o_isnode = B.take(size_t(n) * 4),
                 o_nid = B.take(size_t(n) * 4), o_cf = B.take(n), o_words = B.take(W_WORDS * 4);
    uint8_t* cbuf = static_cast<uint8_t*>(ctx->scratch(TDX_S_A, B.off));
    if (!cbuf) return TDX_ERR_NOMEM;
    ds.workspace_bytes = int64_t(B.off);
    int32_t* inflow = reinterpret_cast<int32_t*>(cbuf + o_inflow);
    uint2 *st_a = reinterpret_cast<uint2*>(cbuf + o_sa), *st_b = reinterpret_cast<uint2*>(cbuf + o_sb);
    int32_t* owin = reinterpret_cast<int32_t*>(cbuf + o_owin);
    uint32_t *isnode = reinterpret_cast<uint32_t*>(cbuf + o_isnode), *nid = reinterpret_cast<uint32_t*>(cbuf + o_nid), *words = reinterpret_cast<uint32_t*>(cbuf + o_words);
    uint8_t* cf = cbuf + o_cf;
    TDX_HIP_CHECK(ctx, hipMemsetAsync(inflow, 0xff, size_t(n) * 32, s));
    TDX_HIP_CHECK(ctx, hipMemsetAsync(owin, 0xff, size_t(n) * 4, s));
    TDX_HIP_CHECK(ctx, hipMemsetAsync(words, 0, W_WORDS * 4, s));

    // ---- outlets onto the cells, inflow table, classes
    const int32_t* d_ids = nullptr;
    if (nout) {
        int32_t* ob = static_cast<int32_t*>(ctx->scratch(TDX_S_K, size_t(nout) * 12));
        if (!ob) return TDX_ERR_NOMEM;
        ds.workspace_bytes += int64_t(size_t(nout) * 12);
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(ob, outlet_x, size_t(nout) * 4, hipMemcpyHostToDevice, s));
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(ob + nout, outlet_y, size_t(nout) * 4, hipMemcpyHostToDevice, s));
        if (outlet_id) {
            TDX_HIP_CHECK(ctx, hipMemcpyAsync(ob + 2 * size_t(nout), outlet_id, size_t(nout) * 4, hipMemcpyHostToDevice, s));
            d_ids = ob + 2 * size_t(nout);
        }
        hipLaunchKernelGGL(outlet_kernel, dim3(tdx_blocks_for(nout, TPB)), dim3(TPB), 0, s, C, ob, ob + nout, nout, nx, ny, owin);
    }
    hipLaunchKernelGGL(inflow_kernel, dim3(cb), dim3(TPB), 0, s, C, inflow);
    hipLaunchKernelGGL(classify_kernel, dim3(cb), dim3(TPB), 0, s, C, inflow, owin, cf, isnode, st_a, d_label, d_order);
    if ((rc = scan32(isnode, nid, n)) != TDX_OK) return rc;
    hipLaunchKernelGGL(total_kernel, dim3(1), dim3(1), 0, s, isnode, nid, n, words + W_NODES);
    if ((rc = lap(DLINK_CLASSIFY)) != TDX_OK) return rc;   // (also: the outlet lists are the caller's)

    // ---- jump: at most ceil(log2(n)) + 1 rounds
    int bound = 1;
    while ((1ull << (bound - 1)) < uint64_t(n)) bound++;
    if (bound > MAX_JUMP) bound = MAX_JUMP;   // (n < 2^31: bound <= 32)
    uint2 *cur = st_a, *other = st_b;
    for (int k = 0; k < bound; k++) {
        hipLaunchKernelGGL(jump_kernel, dim3(cb), dim3(TPB), 0, s, cf, cur, other, n, words + W_JUMP + k);
        std::swap(cur, other);
        ds.jump_rounds++;
        if ((k & 1) || k == bound - 1) {
            if ((rc = read_words(words + W_JUMP, k + 1)) != TDX_OK) return rc;
            bool still = false;
            for (int i = 0; i <= k; i++) still = still || mail[i] == 0;
            if (still) break;
        }
    }
    if ((rc = read_words(words, 1)) != TDX_OK) return rc;
    const uint32_t nn = mail[W_NODES];
    if ((rc = lap(DLINK_JUMP)) != TDX_OK) return rc;
    if (nn > n) { err = "streamnet links: impossible node count"; return TDX_ERR_HIP; }
    if (nn == 0) return TDX_OK;   // nothing but cycles of cells with one inflow: no link

    // ---- the node-sized workspace
    Bump NB;
    const size_t m4 = size_t(nn) * 4, m8 = size_t(nn) * 8;
    const size_t o_cell = NB.take(m4), o_src = NB.take(m4 * 8), o_dist = NB.take(m4 * 8), o_stamp = NB.take(m4), o_h = NB.take(m4), o_root = NB.take(m4), o_ord = NB.take(m4),
                 o_mag = NB.take(m8), o_perm = NB.take(m4), o_cnt = NB.take(m4), o_base = NB.take(m4), o_ka = NB.take(m8), o_kb = NB.take(m8), o_va = NB.take(m4),
                 o_vb = NB.take(m4), o_cs = NB.take(m4), o_bs = NB.take(m4);
    uint8_t* nb = static_cast<uint8_t*>(ctx->scratch(TDX_S_B, NB.off));
    if (!nb) return TDX_ERR_NOMEM;
    ds.workspace_bytes += int64_t(NB.off);
    auto nu32 = [&](size_t o) { return reinterpret_cast<uint32_t*>(nb + o); };
    auto ni32 = [&](size_t o) { return reinterpret_cast<int32_t*>(nb + o); };
    const Nodes N{ni32(o_cell), ni32(o_src), nu32(o_dist), ni32(o_stamp), nu32(o_h), nu32(o_root), ni32(o_ord), reinterpret_cast<long long*>(nb + o_mag), nu32(o_perm),
                  nu32(o_cnt), nu32(o_base)};
    const unsigned nbk = tdx_blocks_for(nn, TPB);
    TDX_HIP_CHECK(ctx, hipMemsetAsync(N.perm, 0, m4, s));
    hipLaunchKernelGGL(node_kernel, dim3(cb), dim3(TPB), 0, s, n, inflow, cf, nid, cur, N);

    // ---- level: a node per link start; rounds until one finishes nothing (at most nn + 1)
    uint32_t done_seen = 0;
    for (uint64_t r = 1; r <= uint64_t(nn) + 1 && r < 0x7fffffffull; r++) {
        hipLaunchKernelGGL(level_kernel, dim3(nbk), dim3(TPB), 0, s, N, nn, cf, int32_t(r), words + W_DONE);
        ds.level_rounds++;
        if (r == 2 || (r & 3) == 0) {
            if ((rc = read_words(words, 2)) != TDX_OK) return rc;
            const uint32_t d = mail[W_DONE];
            if (d == nn || d == done_seen) break;   // all finished, or the rounds since the last look finished nothing
            done_seen = d;
        }
    }
    if ((rc = lap(DLINK_LEVEL)) != TDX_OK) return rc;

    // ---- number: the finished nodes in (h, root) order, the unfinished ones behind them with no link
    unsigned long long *key_a = reinterpret_cast<unsigned long long*>(nb + o_ka), *key_b = reinterpret_cast<unsigned long long*>(nb + o_kb);
    hipLaunchKernelGGL(count_kernel, dim3(nbk), dim3(TPB), 0, s, N, nn, cf, key_a, nu32(o_va));
    rc = tdx_sort_pairs_u64(ctx, TDX_S_D, reinterpret_cast<const uint64_t*>(key_a), reinterpret_cast<uint64_t*>(key_b), nu32(o_va), nu32(o_vb), nn, 64);
    if (rc != TDX_OK) return rc;
    hipLaunchKernelGGL(sorted_count_kernel, dim3(nbk), dim3(TPB), 0, s, N, nn, nu32(o_vb), nu32(o_cs));
    if ((rc = scan32(nu32(o_cs), nu32(o_bs), nn)) != TDX_OK) return rc;
    hipLaunchKernelGGL(base_kernel, dim3(nbk), dim3(TPB), 0, s, N, nn, nu32(o_vb), nu32(o_cs), nu32(o_bs), words);
    if ((rc = read_words(words, 4)) != TDX_OK) return rc;
    const uint32_t nl = mail[W_LINKS];
    if ((rc = lap(DLINK_NUMBER)) != TDX_OK) return rc;
    if (uint64_t(nl) > uint64_t(nn) * 8) { err = "streamnet links: impossible link count"; return TDX_ERR_HIP; }
    if (nl == 0) return TDX_OK;

    // ---- the link-sized workspace, the tree rows included
    Bump LB;
    const size_t l4 = size_t(nl) * 4, l8 = size_t(nl) * 8;
    const size_t o_u1 = LB.take(l4), o_u2 = LB.take(l4), o_d = LB.take(l4), o_lord = LB.take(l4), o_first = LB.take(l4), o_lmag = LB.take(l8), o_dbl = LB.take(l4),
                 o_lcnt = LB.take(l4), o_shape = LB.take(l8), o_beg = LB.take(l8), o_cr = LB.take(l8), o_begr = LB.take(l8), o_tree = LB.take(l8 * 9);
    uint8_t* lb = static_cast<uint8_t*>(ctx->scratch(TDX_S_C, LB.off));
    if (!lb) return TDX_ERR_NOMEM;
    ds.workspace_bytes += int64_t(LB.off);
    auto li32 = [&](size_t o) { return reinterpret_cast<int32_t*>(lb + o); };
    auto lu64 = [&](size_t o) { return reinterpret_cast<unsigned long long*>(lb + o); };
    const LinkArrays L{li32(o_u1), li32(o_u2), li32(o_d), li32(o_lord), li32(o_first), reinterpret_cast<long long*>(lb + o_lmag), reinterpret_cast<uint32_t*>(lb + o_dbl),
                       reinterpret_cast<uint32_t*>(lb + o_lcnt), lu64(o_shape), lu64(o_beg)};
    const unsigned lbk = tdx_blocks_for(nl, TPB);
    TDX_HIP_CHECK(ctx, hipMemsetAsync(lb + o_u1, 0xff, o_lord - o_u1, s));   // u1, u2, d = -1
    TDX_HIP_CHECK(ctx, hipMemsetAsync(lb + o_lord, 0, o_beg - o_lord, s));   // (every link is written by the node that creates it; shape = none)
    hipLaunchKernelGGL(links_init_kernel, dim3(nbk), dim3(TPB), 0, s, N, nn, cf, owin, d_ids, L, nl, d_label, d_order);
    hipLaunchKernelGGL(links_end_kernel, dim3(nbk), dim3(TPB), 0, s, N, nn, cf, owin, d_ids, L, nl);
    hipLaunchKernelGGL(cells_kernel, dim3(cb), dim3(TPB), 0, s, n, cf, cur, nid, N, owin, d_ids, L, nl, d_label, d_order);
    if ((rc = lap(DLINK_LINKS)) != TDX_OK) return rc;

    // ---- rows
    long long* d_tree = reinterpret_cast<long long*>(lb + o_tree);
    hipLaunchKernelGGL(rev_count_kernel, dim3(lbk), dim3(TPB), 0, s, L, nl, lu64(o_cr));
    {
        size_t bytes = 0;
        TDX_HIP_CHECK(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, lu64(o_cr), lu64(o_begr), nl, s));
        void* t = temp(bytes);
        if (!t) return TDX_ERR_NOMEM;
        TDX_HIP_CHECK(ctx, hipcub::DeviceScan::ExclusiveSum(t, bytes, lu64(o_cr), lu64(o_begr), nl, s));
    }
    hipLaunchKernelGGL(tree_kernel, dim3(lbk), dim3(TPB), 0, s, L, nl, lu64(o_begr), d_tree, words);
    if ((rc = read_words(words, 6)) != TDX_OK) return rc;
    const uint64_t np = *reinterpret_cast<const uint64_t*>(mail + W_POINTS);
    if (np < nl || np > uint64_t(n) + 3 * uint64_t(nl)) { err = "streamnet links: impossible point count"; return TDX_ERR_HIP; }
    double* d_coord = static_cast<double*>(ctx->scratch(TDX_S_J, size_t(np) * 40));
    if (!d_coord) return TDX_ERR_NOMEM;
    ds.workspace_bytes += int64_t(size_t(np) * 40 + tmp_max);
    const Geo g{nx, gt[0], gt[1], gt[2], gt[3], dxA * dyA, np};
    hipLaunchKernelGGL(coord_first_kernel, dim3(lbk), dim3(TPB), 0, s, C, g, L, nl, d_coord);
    hipLaunchKernelGGL(coord_node_kernel, dim3(nbk), dim3(TPB), 0, s, C, g, N, nn, L, nl, d_coord);
    hipLaunchKernelGGL(coord_cell_kernel, dim3(cb), dim3(TPB), 0, s, C, g, cf, cur, nid, N, L, nl, d_coord);
    if ((rc = lap(DLINK_ROWS)) != TDX_OK) return rc;

    // ---- the rows to the host
    try {
        out.tree.resize(size_t(nl) * 9);
        out.coord.resize(size_t(np) * 5);
    } catch (const std::bad_alloc&) {
        out = Links();
        err = "streamnet links: out of host memory for the rows";
        return TDX_ERR_NOMEM;
    }
    static_assert(sizeof(long long) == sizeof(int64_t), "tree rows");
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(out.tree.data(), d_tree, size_t(nl) * 72, hipMemcpyDeviceToHost, s));
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(out.coord.data(), d_coord, size_t(np) * 40, hipMemcpyDeviceToHost, s));
    if ((rc = lap(DLINK_DOWNLOAD)) != TDX_OK) return rc;
    TDX_HIP_CHECK(ctx, hipGetLastError());
    return TDX_OK;
}

}  // namespace streamnet
