// The SINMAP parameter region grid on gfx950 (the toolbox step "Create Parameter Region Grid", pyfiles/SIRegionTool.py: gdal.RasterizeLayer or
// gdal.Warp in the reference).  The definition is in include/taudem_amd_regions.h.
//
// Polygon mode.  The host turns the rings into non-horizontal edges in pixel coordinates, counts the rows every edge crosses (clipped to the owned
// rows), scans the counts and gives every feature the box of its clipped rows and word-aligned columns.  Features go to the device in batches whose
// boxes fit the workspace bound.  Per batch:
//   cross   one thread per (edge, row) pair, found by a search in the scanned counts: the crossing xs toggles the bit of the first column whose
//           centre lies right of it (atomicXor on a 32-bit word of the feature's parity bitmap; clamped to column 0, dropped past the box)
//   fill    one wave per (feature, row): a prefix xor within every word by shifts, across the 64 words of a chunk by a ballot, a carried parity
//           across chunks; the inside bits raise the cell's winner word to the feature's index + 1 (atomicMax), 64 consecutive cells per step
// then one streaming pass turns winner -> value (int16, 16-byte stores where the output is aligned) and ORs the values' bits into a presence bitmap
// in LDS, written out once per block.  xor, max and or on integers commute: a run gives the same bytes every time.
// Resample mode is that streaming pass with a gather instead of the winner word, after a pass that only counts the values out of range; constant
// mode is that pass with the value 1.  -ffp-contract=off (the Makefile's HIPFLAGS): the contract's expressions are evaluated as written.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "context.hpp"
#include "device_common.hpp"
#include "region_table.hpp"
#include "strips.hpp"

namespace {

constexpr int64_t DEFAULT_WORKSPACE_WORDS = int64_t(1) << 24;
constexpr int PRESENCE_WORDS = 1024;   // 32768 bits
constexpr int CELLS = 8, BLOCK_CELLS = 256 * CELLS;

struct Edge { double x1, y1, x2, y2; };   // pixel coordinates, y1 != y2
struct Feat {
    int64_t word0;    // the first word of its bitmap in the batch's workspace
    int64_t item0;    // the first (feature, row) item of the batch that is its
    int32_t r_lo, r_n;   // its rows among the owned rows
    int32_t w_lo, w_n;   // its words of a row
    uint32_t index;   // layer index + 1: what the winner word holds
    uint32_t pad;
};

__host__ __device__ inline double clampd(double v, double lo, double hi) { return v < lo ? lo : v > hi ? hi : v; }
// the first integer k with k + 0.5 >= v / with k + 0.5 > v (v finite and far inside the integers a double holds: k + 0.5 is exact)
__host__ __device__ inline int64_t first_centre_at_or_right(double v) { const double k = floor(v); return k + 0.5 >= v ? int64_t(k) : int64_t(k) + 1; }
__host__ __device__ inline int64_t first_centre_right(double v) { const double k = floor(v); return k + 0.5 > v ? int64_t(k) : int64_t(k) + 1; }
// the rows [first, end) of rows [row_lo, row_hi) whose scanline the edge crosses: min(y1, y2) <= r + 0.5 < max(y1, y2)
__host__ __device__ inline void edge_rows(double y1, double y2, int64_t row_lo, int64_t row_hi, int64_t* first, int64_t* end) {
    const double lo = double(row_lo) - 2.0, hi = double(row_hi) + 2.0;
    const int64_t a = first_centre_at_or_right(clampd(y1 < y2 ? y1 : y2, lo, hi)), b = first_centre_at_or_right(clampd(y1 < y2 ? y2 : y1, lo, hi));
    *first = a < row_lo ? row_lo : a > row_hi ? row_hi : a;
    *end = b < row_lo ? row_lo : b > row_hi ? row_hi : b;
}

__global__ __launch_bounds__(256) void cross_kernel(const Edge* __restrict__ edges, const int32_t* __restrict__ efeat, const unsigned long long* __restrict__ pair_off,
                                                    int64_t e0, int64_t e1, unsigned long long p0, unsigned long long n_pairs, const Feat* __restrict__ feats,
                                                    uint32_t* __restrict__ bitmap, int64_t bitmap_words, int64_t row_lo, int64_t row_hi) {
    const unsigned long long k = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (k >= n_pairs) return;
    const unsigned long long p = p0 + k;
    int64_t lo = e0, hi = e1;   // the last edge of [e0, e1) whose first pair is <= p (every edge has at least one pair)
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (pair_off[mid] <= p) lo = mid; else hi = mid;
    }
    const Edge ed = edges[lo];
    int64_t first, end;
    edge_rows(ed.y1, ed.y2, row_lo, row_hi, &first, &end);
    const int64_t r = first + int64_t(p - pair_off[lo]);
    if (r >= end) return;
    const double yc = double(r) + 0.5;
    const double xs = ed.x1 + (yc - ed.y1) * (ed.x2 - ed.x1) / (ed.y2 - ed.y1);
    const Feat f = feats[efeat[lo]];
    const int64_t col_end = (int64_t(f.w_lo) + f.w_n) * 32;
    if (!(xs < double(col_end - 1) + 0.5)) return;   // no column of the box has its centre right of xs (a NaN lands here too)
    int64_t t = xs < 0.5 ? 0 : first_centre_right(xs);
    if (t < int64_t(f.w_lo) * 32) t = int64_t(f.w_lo) * 32;
    const int64_t rr = (r - row_lo) - f.r_lo;
    if (rr < 0 || rr >= f.r_n || t >= col_end) return;
    const int64_t word = f.word0 + rr * f.w_n + ((t >> 5) - f.w_lo);
    if (word < 0 || word >= bitmap_words) return;
    atomicXor(&bitmap[word], 1u << (unsigned(t) & 31u));
}

__global__ __launch_bounds__(256) void fill_kernel(const Feat* __restrict__ feats, int64_t f0, int64_t f1, int64_t n_items, const uint32_t* __restrict__ bitmap,
                                                   uint32_t* __restrict__ winner, int64_t nx) {
    const int64_t item = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (item >= n_items) return;   // a whole wave
    int64_t lo = f0, hi = f1;
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (feats[mid].item0 <= item) lo = mid; else hi = mid;
    }
    const Feat f = feats[lo];
    const int64_t rr = item - f.item0;
    if (rr >= f.r_n) return;
    const uint32_t* row = bitmap + f.word0 + rr * f.w_n;
    uint32_t* win = winner + (int64_t(f.r_lo) + rr) * nx;
    unsigned carry = 0;
    for (int base = 0; base < f.w_n; base += 64) {
        const int wi = base + lane;
        uint32_t x = wi < f.w_n ? row[wi] : 0u;
        if (carry == 0 && __ballot(x != 0) == 0) continue;
        x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8; x ^= x << 16;   // bit i = xor of the toggles 0 .. i
        const unsigned long long odd = __ballot((x >> 31) != 0);
        const unsigned before = unsigned(__popcll(odd & ((1ull << lane) - 1ull))) & 1u;
        if (before ^ carry) x = ~x;
        carry ^= unsigned(__popcll(odd)) & 1u;
        if (wi >= f.w_n) x = 0;
        const int nw = f.w_n - base < 64 ? f.w_n - base : 64;
        for (int j = 0; j < nw; j += 2) {   // 64 consecutive cells per step: the bits of two words
            const int src = j + (lane >> 5);
            const uint32_t xw = __shfl(x, src, 64);
            if (__ballot(xw != 0) == 0) continue;
            const int64_t col = (int64_t(f.w_lo) + base + src) * 32 + (lane & 31);
            if (((xw >> (lane & 31)) & 1u) && col < nx) atomicMax(&win[col], f.index);
        }
    }
}

struct WinnerValue {   // polygon mode: the winner word's feature -> its value
    const uint32_t* winner;
    const int16_t* values;
    __device__ int32_t operator()(int64_t i) const { const uint32_t k = winner[i]; return k ? int32_t(values[k - 1]) : 0; }
};
struct ConstantValue {
    __device__ int32_t operator()(int64_t) const { return 1; }
};
struct ResampleValue {   // the contract's expressions, in its order
    const int32_t* src;
    int64_t snx, sny, nx, row_lo;
    double g0, g1, g3, g5, s0, s1, s3, s5;
    int32_t nd;
    __device__ int32_t operator()(int64_t i) const {
        const uint32_t q = uint32_t(i) / uint32_t(nx);   // i < 2^32 and nx < 2^31 (too_big): a 32-bit division
        const int64_t c = int64_t(uint32_t(i) - q * uint32_t(nx)), r = row_lo + int64_t(q);
        const double x = g0 + (double(c) + 0.5) * g1, y = g3 + (double(r) + 0.5) * g5;
        const double sc = floor((x - s0) / s1), sr = floor((y - s3) / s5);
        if (!(sc >= 0.0 && sc < double(snx) && sr >= 0.0 && sr < double(sny))) return 0;
        const int32_t v = src[int64_t(sr) * snx + int64_t(sc)];
        return v == nd ? 0 : v == 0 ? -1 : v;   // a taken 0 is a value outside 1 .. 32767 like any other
    }
};

using i16x8 = int16_t __attribute__((ext_vector_type(8)));

// WRITE: the values of the owned cells as int16 and the presence bitmap; else only the count of values outside 1 .. 32767 (0 is "no value")
template <class F, bool WRITE>
__global__ __launch_bounds__(256) void value_kernel(F value, int16_t* __restrict__ out, int64_t n, uint32_t* __restrict__ presence, unsigned long long* __restrict__ bad,
                                                    int vec) {
    __shared__ uint32_t s_pres[PRESENCE_WORDS];
    __shared__ unsigned s_bad;
    if (WRITE) for (int k = threadIdx.x; k < PRESENCE_WORDS; k += 256) s_pres[k] = 0;
    else if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    const int64_t i0 = (int64_t(blockIdx.x) * 256 + threadIdx.x) * CELLS;
    if (i0 < n) {
        const int cnt = int(n - i0 < CELLS ? n - i0 : CELLS);
        int16_t v[CELLS];
        unsigned nbad = 0;
        int32_t last = 0;   // a run of one value sets its presence bit once: regions are runs
#pragma unroll
        for (int k = 0; k < CELLS; k++) {
            int32_t a = k < cnt ? value(i0 + k) : 0;
            if (a < 0 || a > 32767) { nbad++; a = 0; }
            v[k] = int16_t(a);
            if (WRITE && a && a != last) atomicOr(&s_pres[a >> 5], 1u << (a & 31));
            last = a;
        }
        if (WRITE) {
            if (vec && cnt == CELLS) {
                i16x8 q;
#pragma unroll
                for (int k = 0; k < CELLS; k++) q[k] = v[k];
                *reinterpret_cast<i16x8*>(out + i0) = q;
            } else {
                for (int k = 0; k < cnt; k++) out[i0 + k] = v[k];
            }
        } else if (nbad) {
            atomicAdd(&s_bad, nbad);
        }
    }
    __syncthreads();
    if (WRITE) {
        for (int k = threadIdx.x; k < PRESENCE_WORDS; k += 256)
            if (s_pres[k]) atomicOr(&presence[k], s_pres[k]);
    } else if (threadIdx.x == 0 && s_bad) {
        atomicAdd(bad, (unsigned long long)s_bad);
    }
}

struct PhaseClock {
    tdx_context* ctx;
    bool on;   // phase times were asked for: only then is the stream drained at a phase's end
    std::chrono::steady_clock::time_point t;
    PhaseClock(tdx_context* c, bool wanted) : ctx(c), on(wanted), t(std::chrono::steady_clock::now()) {}
    int lap(double* ms) {   // adds the wall time since the last lap, with the stream drained
        if (!on) return TDX_OK;
        TDX_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        const auto now = std::chrono::steady_clock::now();
        *ms += std::chrono::duration<double, std::milli>(now - t).count();
        t = now;
        return TDX_OK;
    }
};

// The owned rows of the output: row_lo .. row_lo + ny_own - 1 of the raster, at d_out
struct Target {
    int16_t* d_out;
    int64_t nx, ny_own, row_lo;
    int64_t cells() const { return nx * ny_own; }
};

// The streaming pass and what follows it: presence (and bad) to the host, the ids decoded.  d_flags: PRESENCE_WORDS words + one 64-bit count, zeroed here.
template <class F>
int write_values(tdx_context* ctx, const F& value, const Target& t, uint32_t* d_flags, bool count_first, int32_t* ids, int32_t* n_ids, tdx_stats* stats, const char* who) {
    hipStream_t s = ctx->stream;
    const int64_t n = t.cells();
    const unsigned nblocks = tdx_blocks_for(uint64_t(n), BLOCK_CELLS);
    unsigned long long* d_bad = reinterpret_cast<unsigned long long*>(d_flags + PRESENCE_WORDS);
    const int vec = (reinterpret_cast<uintptr_t>(t.d_out) & 15u) == 0;
    uint32_t h_flags[PRESENCE_WORDS + 2];
    TdxSpan sp(ctx, TDX_K_MISC);
    TDX_HIP_CHECK(ctx, hipMemsetAsync(d_flags, 0, (PRESENCE_WORDS + 2) * 4, s));
    if (count_first) {
        hipLaunchKernelGGL((value_kernel<F, false>), dim3(nblocks), dim3(256), 0, s, value, t.d_out, n, d_flags, d_bad, vec);
        if (stats) stats->launches[TDX_K_MISC] += 1;
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(h_flags + PRESENCE_WORDS, d_bad, 8, hipMemcpyDeviceToHost, s));
        TDX_HIP_CHECK(ctx, hipStreamSynchronize(s));
        unsigned long long bad;
        memcpy(&bad, h_flags + PRESENCE_WORDS, 8);
        if (bad) return tdx_fail(ctx, TDX_ERR_ARG, std::string(who) + ": " + std::to_string(bad) + " cells take a source value outside 1 .. 32767");
    }
    hipLaunchKernelGGL((value_kernel<F, true>), dim3(nblocks), dim3(256), 0, s, value, t.d_out, n, d_flags, d_bad, vec);
    if (stats) stats->launches[TDX_K_MISC] += 1;
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(h_flags, d_flags, PRESENCE_WORDS * 4, hipMemcpyDeviceToHost, s));
    TDX_HIP_CHECK(ctx, hipStreamSynchronize(s));
    int32_t k = 0;
    for (int32_t v = 1; v < PRESENCE_WORDS * 32; v++)
        if ((h_flags[v >> 5] >> (v & 31)) & 1u) { if (ids) ids[k] = v; k++; }
    if (n_ids) *n_ids = k;
    return TDX_OK;
}

struct Batch { int64_t f0, f1, e0, e1, words, items; unsigned long long p0, pairs; };

struct Prepared {
    std::vector<Edge> edges;
    std::vector<int32_t> efeat;              // index into feats
    std::vector<unsigned long long> pair_off;   // edges + 1
    std::vector<Feat> feats;                 // the features that have a box, in layer order
    std::vector<int16_t> values;             // of all features, by layer index
    std::vector<Batch> batches;
    int64_t max_words = 0;
};

bool ring_counts(const double* x, const double* y, int64_t v0, int64_t v1) {   // at least 3 distinct vertices
    int64_t a = -1;
    for (int64_t i = v0 + 1; i < v1; i++) {
        if (x[i] == x[v0] && y[i] == y[v0]) continue;
        if (a < 0) { a = i; continue; }
        if (x[i] == x[a] && y[i] == y[a]) continue;
        return true;
    }
    return false;
}

int prepare(const double* x, const double* y, const int64_t* ring_first, int64_t n_rings, const int64_t* feature_first, const int32_t* values, int64_t n_features,
            const double* gt, int64_t ws_words, const Target& t, Prepared& P, std::string& err) {
    if (feature_first[0] != 0 || ring_first[0] != 0 || feature_first[n_features] != n_rings) { err = "the offsets of the rings do not cover them"; return TDX_ERR_ARG; }
    for (int64_t f = 0; f < n_features; f++) {
        if (feature_first[f + 1] < feature_first[f]) { err = "feature offsets that descend"; return TDX_ERR_ARG; }
        if (values[f] < 1 || values[f] > 32767) {
            err = "feature " + std::to_string(f) + ": value " + std::to_string(values[f]) + " is outside 1 .. 32767";
            return TDX_ERR_ARG;
        }
    }
    for (int64_t q = 0; q < n_rings; q++)
        if (ring_first[q + 1] < ring_first[q]) { err = "ring offsets that descend"; return TDX_ERR_ARG; }
    if (n_features > int64_t(0x7ffffff0)) { err = "too many features"; return TDX_ERR_ARG; }
    const int64_t row_lo = t.row_lo, row_hi = t.row_lo + t.ny_own;
    P.values.resize(size_t(n_features));
    P.pair_off.push_back(0);
    unsigned long long pairs = 0;
    Batch b{0, 0, 0, 0, 0, 0, 0, 0};
    auto close_batch = [&](size_t e_end) {
        b.f1 = int64_t(P.feats.size()); b.e1 = int64_t(e_end); b.pairs = pairs - b.p0;
        if (b.f1 > b.f0) { P.batches.push_back(b); P.max_words = std::max(P.max_words, b.words); }
        b = Batch{b.f1, b.f1, b.e1, b.e1, 0, 0, pairs, 0};
    };
    for (int64_t f = 0; f < n_features; f++) {
        P.values[size_t(f)] = int16_t(values[f]);
        const size_t e_start = P.edges.size();
        double xmin = INFINITY, xmax = -INFINITY;
        int64_t r_lo = row_hi, r_hi = row_lo;
        for (int64_t q = feature_first[f]; q < feature_first[f + 1]; q++) {
            const int64_t v0 = ring_first[q], v1 = ring_first[q + 1];
            if (v1 - v0 < 3 || !ring_counts(x, y, v0, v1)) continue;
            for (int64_t i = v0; i < v1; i++) {
                const int64_t j = i + 1 < v1 ? i + 1 : v0;   // the last vertex back to the first: no edge when they are equal (y1 == y2)
                Edge e;
                e.x1 = (x[i] - gt[0]) / gt[1]; e.y1 = (y[i] - gt[3]) / gt[5];
                e.x2 = (x[j] - gt[0]) / gt[1]; e.y2 = (y[j] - gt[3]) / gt[5];
                if (!(std::isfinite(e.x1) && std::isfinite(e.y1) && std::isfinite(e.x2) && std::isfinite(e.y2))) {
                    err = "feature " + std::to_string(f) + ": a vertex without finite pixel coordinates";
                    return TDX_ERR_ARG;
                }
                if (e.y1 == e.y2) continue;
                int64_t first, end;
                edge_rows(e.y1, e.y2, row_lo, row_hi, &first, &end);
                if (end <= first) continue;
                xmin = std::min(xmin, std::min(e.x1, e.x2)); xmax = std::max(xmax, std::max(e.x1, e.x2));
                r_lo = std::min(r_lo, first); r_hi = std::max(r_hi, end);
                P.edges.push_back(e);
            }
        }
        if (P.edges.size() == e_start) continue;
        // one column of slack on either side: xs may leave [xmin, xmax] by a rounding
        const double lim = double(t.nx) + 2.0;
        const int64_t c_lo = std::max<int64_t>(0, first_centre_right(clampd(xmin, -2.0, lim)) - 1);
        const int64_t c_end = std::min<int64_t>(t.nx, first_centre_right(clampd(xmax, -2.0, lim)) + 1);
        if (c_end <= c_lo) { P.edges.resize(e_start); continue; }   // left or right of the raster: an even number of crossings left of every centre
        Feat F;
        F.r_lo = int32_t(r_lo - row_lo); F.r_n = int32_t(r_hi - r_lo);
        F.w_lo = int32_t(c_lo >> 5); F.w_n = int32_t(((c_end + 31) >> 5) - (c_lo >> 5));
        F.index = uint32_t(f) + 1; F.pad = 0;
        const int64_t words = int64_t(F.r_n) * F.w_n;
        if (b.words > 0 && b.words + words > ws_words) close_batch(e_start);   // this feature opens the next batch: its edges are not in b
        F.word0 = b.words; F.item0 = b.items;
        b.words += words; b.items += F.r_n;
        const int32_t fi = int32_t(P.feats.size());
        P.feats.push_back(F);
        for (size_t k = e_start; k < P.edges.size(); k++) {
            int64_t first, end;
            edge_rows(P.edges[k].y1, P.edges[k].y2, row_lo, row_hi, &first, &end);
            pairs += (unsigned long long)(end - first);
            P.efeat.push_back(fi);
            P.pair_off.push_back(pairs);
        }
    }
    close_batch(P.edges.size());
    return TDX_OK;
}

int polygons_impl(tdx_context* ctx, const double* x, const double* y, const int64_t* ring_first, int64_t n_rings, const int64_t* feature_first, const int32_t* values,
                  int64_t n_features, const double* gt, int64_t ws_words, const Target& t, int32_t* ids, int32_t* n_ids, double* phase_ms, int64_t* ws_bytes,
                  tdx_stats* stats, const char* who) {
    if (gt[2] != 0.0 || gt[4] != 0.0) return tdx_fail(ctx, TDX_ERR_ARG, std::string(who) + ": a rotated geotransform is not supported");
    if (!(gt[1] != 0.0 && gt[5] != 0.0)) return tdx_fail(ctx, TDX_ERR_ARG, std::string(who) + ": a geotransform without a cell size");
    if (ws_words <= 0) ws_words = DEFAULT_WORKSPACE_WORDS;
    double ms[TDX_REGIONGRID_PHASES] = {0, 0, 0, 0};
    TDX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    PhaseClock clock(ctx, phase_ms != nullptr);
    Prepared P;
    std::string err;
    int rc;
    try {
        rc = prepare(x, y, ring_first, n_rings, feature_first, values, n_features, gt, ws_words, t, P, err);
    } catch (const std::bad_alloc&) {
        return tdx_fail(ctx, TDX_ERR_NOMEM, std::string(who) + ": out of host memory for the edges");
    }
    if (rc != TDX_OK) return tdx_fail(ctx, rc, std::string(who) + ": " + err);
    const size_t ne = P.edges.size(), nf = P.feats.size(), nv = P.values.size();
    const size_t n_cells = size_t(t.cells());
    const size_t bytes_win = n_cells * 4, bytes_bits = size_t(std::max<int64_t>(P.max_words, 1)) * 4, bytes_e = ne * sizeof(Edge) + 16,
                 bytes_ef = ne * 4 + 16, bytes_po = (ne + 1) * 8, bytes_f = nf * sizeof(Feat) + 16, bytes_v = nv * 2 + 16, bytes_fl = (PRESENCE_WORDS + 2) * 4;
    uint32_t* d_win = static_cast<uint32_t*>(ctx->scratch(TDX_S_A, bytes_win));
    uint32_t* d_bits = static_cast<uint32_t*>(ctx->scratch(TDX_S_B, bytes_bits));
    Edge* d_edges = static_cast<Edge*>(ctx->scratch(TDX_S_C, bytes_e));
    int32_t* d_efeat = static_cast<int32_t*>(ctx->scratch(TDX_S_D, bytes_ef));
    unsigned long long* d_off = static_cast<unsigned long long*>(ctx->scratch(TDX_S_E, bytes_po));
    Feat* d_feats = static_cast<Feat*>(ctx->scratch(TDX_S_F, bytes_f));
    int16_t* d_values = static_cast<int16_t*>(ctx->scratch(TDX_S_G, bytes_v));
    uint32_t* d_flags = static_cast<uint32_t*>(ctx->scratch(TDX_S_H, bytes_fl));
    if (!d_win || !d_bits || !d_edges || !d_efeat || !d_off || !d_feats || !d_values || !d_flags) return TDX_ERR_NOMEM;
    if (ws_bytes) *ws_bytes = int64_t(bytes_win + bytes_bits + bytes_e + bytes_ef + bytes_po + bytes_f + bytes_v + bytes_fl);
    ctx->begin_call(stats);
    ctx->stage = who;
    {
        TdxSpan sp(ctx, TDX_K_MISC);
        if (ne) {
            TDX_HIP_CHECK(ctx, hipMemcpyAsync(d_edges, P.edges.data(), ne * sizeof(Edge), hipMemcpyHostToDevice, s));
            TDX_HIP_CHECK(ctx, hipMemcpyAsync(d_efeat, P.efeat.data(), ne * 4, hipMemcpyHostToDevice, s));
            TDX_HIP_CHECK(ctx, hipMemcpyAsync(d_feats, P.feats.data(), nf * sizeof(Feat), hipMemcpyHostToDevice, s));
        }
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(d_off, P.pair_off.data(), (ne + 1) * 8, hipMemcpyHostToDevice, s));
        if (nv) TDX_HIP_CHECK(ctx, hipMemcpyAsync(d_values, P.values.data(), nv * 2, hipMemcpyHostToDevice, s));
        TDX_HIP_CHECK(ctx, hipMemsetAsync(d_win, 0, bytes_win, s));
    }
    if ((rc = clock.lap(&ms[TDX_REGIONGRID_PREPARE])) != TDX_OK) return rc;
    for (const Batch& b : P.batches) {
        if (b.pairs > 0xffffffffull * 256ull || b.items > int64_t(0x7fffffff) * 4) return tdx_fail(ctx, TDX_ERR_ARG, std::string(who) + ": too many crossings in one batch");
        {
            TdxSpan sp(ctx, TDX_K_ACCUM);
            TDX_HIP_CHECK(ctx, hipMemsetAsync(d_bits, 0, size_t(b.words) * 4, s));
            if (b.pairs) {
                hipLaunchKernelGGL(cross_kernel, dim3(tdx_blocks_for(b.pairs, 256)), dim3(256), 0, s, d_edges, d_efeat, d_off, b.e0, b.e1, b.p0, b.pairs, d_feats, d_bits,
                                   b.words, t.row_lo, t.row_lo + t.ny_own);
                if (stats) stats->launches[TDX_K_ACCUM] += 1;
            }
        }
        if ((rc = clock.lap(&ms[TDX_REGIONGRID_CROSS])) != TDX_OK) return rc;
        {
            TdxSpan sp(ctx, TDX_K_STENCIL);
            hipLaunchKernelGGL(fill_kernel, dim3(tdx_blocks_for(uint64_t(b.items), 4)), dim3(256), 0, s, d_feats, b.f0, b.f1, b.items, d_bits, d_win, t.nx);
            if (stats) stats->launches[TDX_K_STENCIL] += 1;
        }
        if ((rc = clock.lap(&ms[TDX_REGIONGRID_FILL])) != TDX_OK) return rc;
    }
    WinnerValue value{d_win, d_values};
    if ((rc = write_values(ctx, value, t, d_flags, false, ids, n_ids, stats, who)) != TDX_OK) return rc;
    if ((rc = clock.lap(&ms[TDX_REGIONGRID_WRITE])) != TDX_OK) return rc;
    TDX_HIP_CHECK(ctx, hipGetLastError());
    ctx->end_call();
    if (phase_ms) memcpy(phase_ms, ms, sizeof ms);
    return TDX_OK;
}

int resample_impl(tdx_context* ctx, const int32_t* d_src, int64_t snx, int64_t sny, const double* sgt, int32_t nd, const double* gt, const Target& t, int32_t* ids,
                  int32_t* n_ids, double* phase_ms, tdx_stats* stats, const char* who) {
    if (gt[2] != 0.0 || gt[4] != 0.0 || sgt[2] != 0.0 || sgt[4] != 0.0) return tdx_fail(ctx, TDX_ERR_ARG, std::string(who) + ": a rotated geotransform is not supported");
    if (!(sgt[1] != 0.0 && sgt[5] != 0.0)) return tdx_fail(ctx, TDX_ERR_ARG, std::string(who) + ": a source geotransform without a cell size");
    double ms[TDX_REGIONGRID_PHASES] = {0, 0, 0, 0};
    TDX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    uint32_t* d_flags = static_cast<uint32_t*>(ctx->scratch(TDX_S_H, (PRESENCE_WORDS + 2) * 4));
    if (!d_flags) return TDX_ERR_NOMEM;
    ctx->begin_call(stats);
    ctx->stage = who;
    PhaseClock clock(ctx, phase_ms != nullptr);
    ResampleValue value{d_src, snx, sny, t.nx, t.row_lo, gt[0], gt[1], gt[3], gt[5], sgt[0], sgt[1], sgt[3], sgt[5], nd};
    int rc;
    if ((rc = write_values(ctx, value, t, d_flags, true, ids, n_ids, stats, who)) != TDX_OK) return rc;
    if ((rc = clock.lap(&ms[TDX_REGIONGRID_WRITE])) != TDX_OK) return rc;
    TDX_HIP_CHECK(ctx, hipGetLastError());
    ctx->end_call();
    if (phase_ms) memcpy(phase_ms, ms, sizeof ms);
    return TDX_OK;
}

int constant_impl(tdx_context* ctx, const Target& t, int32_t* ids, int32_t* n_ids, tdx_stats* stats, const char* who) {
    TDX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    uint32_t* d_flags = static_cast<uint32_t*>(ctx->scratch(TDX_S_H, (PRESENCE_WORDS + 2) * 4));
    if (!d_flags) return TDX_ERR_NOMEM;
    ctx->begin_call(stats);
    ctx->stage = who;
    int rc;
    if ((rc = write_values(ctx, ConstantValue{}, t, d_flags, false, ids, n_ids, stats, who)) != TDX_OK) return rc;
    TDX_HIP_CHECK(ctx, hipGetLastError());
    ctx->end_call();
    return TDX_OK;
}

bool bad_polygons(const double* x, const double* y, const int64_t* ring_first, int64_t n_rings, const int64_t* feature_first, const int32_t* values, int64_t n_features,
                  const double* gt) {
    if (!ring_first || !feature_first || !gt || n_rings < 0 || n_features < 0 || (n_features > 0 && !values)) return true;
    return ring_first[n_rings] > 0 && (!x || !y);
}
bool bad_strip(int64_t nx, int64_t ny_local, int64_t row0, int64_t ny_total) { return nx <= 0 || ny_local <= 0 || row0 < 0 || ny_total < row0 + ny_local; }
const char* const kTooBig = "raster larger than 2^32 cells per device strip";

}  // namespace

extern "C" int tdx_regiongrid_dev(tdx_context* ctx, const double* x, const double* y, const int64_t* ring_first, int64_t n_rings, const int64_t* feature_first,
                                  const int32_t* values, int64_t n_features, const double* gt, int64_t workspace_words, int64_t nx, int64_t ny, int16_t* d_out,
                                  int32_t* ids, int32_t* n_ids, double* phase_ms, int64_t* workspace_bytes, tdx_stats* stats) {
    if (!ctx || !d_out || nx <= 0 || ny <= 0 || bad_polygons(x, y, ring_first, n_rings, feature_first, values, n_features, gt))
        return tdx_fail(ctx, TDX_ERR_ARG, "tdx_regiongrid_dev: bad argument");
    if (too_big(nx, ny)) return tdx_fail(ctx, TDX_ERR_ARG, kTooBig);
    return polygons_impl(ctx, x, y, ring_first, n_rings, feature_first, values, n_features, gt, workspace_words, Target{d_out, nx, ny, 0}, ids, n_ids, phase_ms,
                         workspace_bytes, stats, "tdx_regiongrid");
}

extern "C" int tdx_regiongrid(tdx_context* ctx, const double* x, const double* y, const int64_t* ring_first, int64_t n_rings, const int64_t* feature_first,
                              const int32_t* values, int64_t n_features, const double* gt, int64_t workspace_words, int64_t nx, int64_t ny, int16_t* out, int32_t* ids,
                              int32_t* n_ids, double* phase_ms, int64_t* workspace_bytes, tdx_stats* stats) {
    if (!ctx || !out || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_regiongrid: bad argument");
    if (too_big(nx, ny)) return tdx_fail(ctx, TDX_ERR_ARG, kTooBig);
    HostCall h(ctx, nx, ny);
    int16_t* d_out = h.out(TDX_S_IO0, out);
    if (h.error) return h.error;
    return h.finish(tdx_regiongrid_dev(ctx, x, y, ring_first, n_rings, feature_first, values, n_features, gt, workspace_words, nx, ny, d_out, ids, n_ids, phase_ms,
                                       workspace_bytes, stats));
}

extern "C" int tdx_regiongrid_strip(tdx_context* ctx, const tdx_comm* /*comm*/, const double* x, const double* y, const int64_t* ring_first, int64_t n_rings,
                                    const int64_t* feature_first, const int32_t* values, int64_t n_features, const double* gt, int64_t workspace_words, int64_t nx,
                                    int64_t ny_local, int64_t row0, int64_t ny_total, int16_t* d_out, int32_t* ids, int32_t* n_ids, double* phase_ms,
                                    int64_t* workspace_bytes, tdx_stats* stats) {
    if (!ctx || !d_out || bad_strip(nx, ny_local, row0, ny_total) || bad_polygons(x, y, ring_first, n_rings, feature_first, values, n_features, gt))
        return tdx_fail(ctx, TDX_ERR_ARG, "tdx_regiongrid_strip: bad argument");
    if (too_big(nx, ny_local + 2) || ny_total > 0x7ffffff0) return tdx_fail(ctx, TDX_ERR_ARG, kTooBig);
    return polygons_impl(ctx, x, y, ring_first, n_rings, feature_first, values, n_features, gt, workspace_words, Target{d_out + nx, nx, ny_local, row0}, ids, n_ids,
                         phase_ms, workspace_bytes, stats, "tdx_regiongrid_strip");
}

extern "C" int tdx_regiongrid_resample_dev(tdx_context* ctx, const int32_t* d_src, int64_t snx, int64_t sny, const double* sgt, int32_t src_nodata, const double* gt,
                                           int64_t nx, int64_t ny, int16_t* d_out, int32_t* ids, int32_t* n_ids, double* phase_ms, tdx_stats* stats) {
    if (!ctx || !d_src || !sgt || !gt || !d_out || snx <= 0 || sny <= 0 || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_regiongrid_resample_dev: bad argument");
    if (too_big(nx, ny) || too_big(snx, sny)) return tdx_fail(ctx, TDX_ERR_ARG, kTooBig);
    return resample_impl(ctx, d_src, snx, sny, sgt, src_nodata, gt, Target{d_out, nx, ny, 0}, ids, n_ids, phase_ms, stats, "tdx_regiongrid_resample");
}

extern "C" int tdx_regiongrid_resample(tdx_context* ctx, const int32_t* src, int64_t snx, int64_t sny, const double* sgt, int32_t src_nodata, const double* gt, int64_t nx,
                                       int64_t ny, int16_t* out, int32_t* ids, int32_t* n_ids, double* phase_ms, tdx_stats* stats) {
    if (!ctx || !src || !out || snx <= 0 || sny <= 0 || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_regiongrid_resample: bad argument");
    if (too_big(nx, ny) || too_big(snx, sny)) return tdx_fail(ctx, TDX_ERR_ARG, kTooBig);
    HostCall hs(ctx, snx, sny);
    const int32_t* d_src = hs.in(TDX_S_IO1, src);
    if (hs.error) return hs.error;
    HostCall h(ctx, nx, ny);
    int16_t* d_out = h.out(TDX_S_IO0, out);
    if (h.error) return h.error;
    return h.finish(tdx_regiongrid_resample_dev(ctx, d_src, snx, sny, sgt, src_nodata, gt, nx, ny, d_out, ids, n_ids, phase_ms, stats));
}

extern "C" int tdx_regiongrid_resample_strip(tdx_context* ctx, const tdx_comm* /*comm*/, const int32_t* d_src, int64_t snx, int64_t sny, const double* sgt,
                                             int32_t src_nodata, const double* gt, int64_t nx, int64_t ny_local, int64_t row0, int64_t ny_total, int16_t* d_out,
                                             int32_t* ids, int32_t* n_ids, double* phase_ms, tdx_stats* stats) {
    if (!ctx || !d_src || !sgt || !gt || !d_out || snx <= 0 || sny <= 0 || bad_strip(nx, ny_local, row0, ny_total))
        return tdx_fail(ctx, TDX_ERR_ARG, "tdx_regiongrid_resample_strip: bad argument");
    if (too_big(nx, ny_local + 2) || too_big(snx, sny) || ny_total > 0x7ffffff0) return tdx_fail(ctx, TDX_ERR_ARG, kTooBig);
    return resample_impl(ctx, d_src, snx, sny, sgt, src_nodata, gt, Target{d_out + nx, nx, ny_local, row0}, ids, n_ids, phase_ms, stats, "tdx_regiongrid_resample_strip");
}

extern "C" int tdx_regiongrid_constant_dev(tdx_context* ctx, int64_t nx, int64_t ny, int16_t* d_out, int32_t* ids, int32_t* n_ids, tdx_stats* stats) {
    if (!ctx || !d_out || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_regiongrid_constant_dev: bad argument");
    if (too_big(nx, ny)) return tdx_fail(ctx, TDX_ERR_ARG, kTooBig);
    return constant_impl(ctx, Target{d_out, nx, ny, 0}, ids, n_ids, stats, "tdx_regiongrid_constant");
}

extern "C" int tdx_regiongrid_constant(tdx_context* ctx, int64_t nx, int64_t ny, int16_t* out, int32_t* ids, int32_t* n_ids, tdx_stats* stats) {
    if (!ctx || !out || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_regiongrid_constant: bad argument");
    if (too_big(nx, ny)) return tdx_fail(ctx, TDX_ERR_ARG, kTooBig);
    HostCall h(ctx, nx, ny);
    int16_t* d_out = h.out(TDX_S_IO0, out);
    if (h.error) return h.error;
    return h.finish(tdx_regiongrid_constant_dev(ctx, nx, ny, d_out, ids, n_ids, stats));
}

extern "C" int tdx_regiongrid_constant_strip(tdx_context* ctx, const tdx_comm* /*comm*/, int64_t nx, int64_t ny_local, int64_t row0, int64_t ny_total, int16_t* d_out,
                                             int32_t* ids, int32_t* n_ids, tdx_stats* stats) {
    if (!ctx || !d_out || bad_strip(nx, ny_local, row0, ny_total)) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_regiongrid_constant_strip: bad argument");
    if (too_big(nx, ny_local + 2)) return tdx_fail(ctx, TDX_ERR_ARG, kTooBig);
    return constant_impl(ctx, Target{d_out + nx, nx, ny_local, row0}, ids, n_ids, stats, "tdx_regiongrid_constant_strip");
}

extern "C" int tdx_regiongrid_write_calpar(const char* path, const int32_t* ids, int32_t n_ids, const char* const* seven_texts) {
    if (!path || n_ids < 0 || (n_ids > 0 && !ids) || !seven_texts) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_regiongrid_write_calpar: bad argument");
    for (int j = 0; j < 7; j++)
        if (!seven_texts[j]) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_regiongrid_write_calpar: bad argument");
    std::string err;
    if (!regions::write_table(path, ids, n_ids, seven_texts, err)) return tdx_fail(nullptr, TDX_ERR_FILE, err);
    return TDX_OK;
}
