// CatchHydroGeo (catchhydrogeo, src/CatchHydroGeo.cpp:69-413) and InunDepth (inundepth, src/InunDepth.cpp:53-545) on gfx950: what consumes a HAND
// raster.  Every cell is independent; the work is a KEYED reduction - per cell up to nheight x 4 accumulators addressed by an arbitrary 32-bit
// catchment id - and a streaming pass for the depth raster.
//
// Keyed reduction (chg_* kernels, DESIGN.md section 4 "CatchHydroGeo and InunDepth"):
//   * id -> list index by binary search in the sorted distinct ids, each with the index of its LAST list row (catchhash[id] = i: last wins).
//   * one 256-thread workgroup owns a 64 x 64 tile, 16 cells per thread in registers (index, hand, cell area, bed term).
//   * the tile walks its distinct indices in ascending order by repeated minimum extraction (a block-wide min over the indices above the
//     previous one): no list of ids is kept, so a tile with 4096 distinct ids just runs 4096 iterations - nothing overflows.
//   * per index and stage: 16 cells in registers in row order, then across the wave by xor shuffles, then the 4 waves through LDS in wave order.
//     The fp64 terms are the reference's expressions; -ffp-contract=off keeps the products and sums apart.
//   * no floating-point atomics: the tile's sums go to a slab record (tile, index); the records are numbered in tile order by an exclusive scan
//     of the per-tile distinct counts (chg_count_kernel), a stable radix sort by index groups them, and chg_reduce_kernel adds each
//     (stage, catchment) over its records in ascending tile order.  The result is a function of the input and the strip cuts only.
//   * the integer cell counts use integer atomics.
//   * stages are processed in chunks of at most HC_MAX, fewer when the slab (records x 3 x chunk x 8 bytes) would pass TDX_CHG_SLAB_MB.
// InunDepth's inundated area is the same reduction with one term and no stage (the catchment-area slot) over the cells that are wet.
#include <algorithm>
#include <numeric>
#include <vector>

#include "context.hpp"
#include "device_common.hpp"
#include "strips.hpp"

int tdx_sort_pairs_u32(tdx_context* ctx, int scratch_slot, const uint32_t* keys_in, uint32_t* keys_out, const uint32_t* vals_in, uint32_t* vals_out, size_t n);

namespace {
using namespace tdxk;

constexpr int TS = 64;         // tile edge
constexpr int CPT = 16;        // cells per thread: column tid & 63, rows (tid >> 6) + 4 i
constexpr int HC_MAX = 128;    // stages per launch: 4 waves x 3 terms x HC_MAX doubles of LDS
constexpr int NONE = 0x7fffffff;

struct Lookup {   // sorted distinct ids and the list row that wins each
    const int32_t* keys;
    const int32_t* win;
    int n;
    __device__ __forceinline__ int find(int32_t id) const {
        int lo = 0, hi = n;
        while (lo < hi) {
            const int m = (lo + hi) >> 1;
            if (keys[m] < id) lo = m + 1; else hi = m;
        }
        return (lo < n && keys[lo] == id) ? win[lo] : -1;
    }
};

struct TileArgs {
    const float* hand;
    const int32_t* cat;
    const float* slp;        // CatchHydroGeo only
    const float* depth;      // InunDepth only: depth per forecast row
    const double* dxc;       // per array row
    const double* dyc;
    Lookup L;
    int nx, y0, y1, tiles_x;
    float hand_nd, slp_nd;
    int32_t cat_nd;
};

// The thread's 16 cells.  ci: list index the cell adds to, -1 for none.  wet (CatchHydroGeo): bit i set where hand and slp have data.
template <bool INUN>
__device__ __forceinline__ void load_cells(const TileArgs& a, int (&ci)[CPT], float (&hv)[CPT], float (&sv)[CPT], unsigned& wet) {
    const int tile = blockIdx.x, tx = tile % a.tiles_x, ty = tile / a.tiles_x;
    const int x = tx * TS + (threadIdx.x & 63);
    int32_t prev_id = 0;
    int prev_ix = -2;
    wet = 0u;
#pragma unroll
    for (int i = 0; i < CPT; i++) {
        const int y = a.y0 + ty * TS + int(threadIdx.x >> 6) + 4 * i;
        ci[i] = -1; hv[i] = 0.f; sv[i] = 0.f;
        if (x >= a.nx || y >= a.y1) continue;
        const size_t c = size_t(y) * size_t(a.nx) + size_t(x);
        const int32_t id = a.cat[c];
        if (id == a.cat_nd) continue;
        const float h = a.hand[c];
        const bool h_ok = !is_nodata_f(h, a.hand_nd);
        if (INUN && !h_ok) continue;
        if (prev_ix == -2 || id != prev_id) { prev_id = id; prev_ix = a.L.find(id); }
        int ix = prev_ix;
        if (INUN && ix >= 0) {
            const float d = a.depth[ix];
            if (!(d > 0) || !((d - h) > 0.0)) ix = -1;
        }
        ci[i] = ix;
        hv[i] = h;
        if (!INUN) {
            const float s = a.slp[c];
            sv[i] = s;
            if (h_ok && !is_nodata_f(s, a.slp_nd)) wet |= 1u << i;
        }
    }
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// the smallest index above `prev` in the tile (NONE: none left); sm: 4 ints of LDS
__device__ __forceinline__ int next_index(const int (&ci)[CPT], int prev, int* sm) {
    int m = NONE;
#pragma unroll
    for (int i = 0; i < CPT; i++) if (ci[i] > prev) m = min(m, ci[i]);
    m = wave_min(m);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    m = min(min(sm[0], sm[1]), min(sm[2], sm[3]));
    __syncthreads();
    return m;
}

template <bool INUN>
__global__ __launch_bounds__(256) void chg_count_kernel(TileArgs a, uint32_t* __restrict__ tcount) {
    __shared__ int sm[4];
    int ci[CPT];
    float hv[CPT], sv[CPT];
    unsigned wet;
    load_cells<INUN>(a, ci, hv, sv, wet);
    uint32_t n = 0;
    for (int prev = -1;;) {
        const int cur = next_index(ci, prev, sm);
        if (cur == NONE) break;
        n++;
        prev = cur;
    }
    if (threadIdx.x == 0) tcount[blockIdx.x] = n;
}

// Stages [k0, k0 + hc) of every record of the tile.  slab: [record][3][hc]; areaslab / keys / vals: [record] (first chunk only).
template <bool INUN>
__global__ __launch_bounds__(256) void chg_tile_kernel(TileArgs a, const uint32_t* __restrict__ toff, const double* __restrict__ height, int k0, int hc, int ncatch, int first,
                                                       double* __restrict__ slab, double* __restrict__ areaslab, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                       int32_t* __restrict__ count) {
    __shared__ int sm[4];
    __shared__ double sRed[4][3 * HC_MAX];
    __shared__ int sCnt[4][HC_MAX];
    __shared__ double sArea[4];
    int ci[CPT];
    float hv[CPT], sv[CPT];
    unsigned wet;
    load_cells<INUN>(a, ci, hv, sv, wet);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ty = blockIdx.x / a.tiles_x;
    double area[CPT], bedt[CPT];
    bool zeroish[CPT];
#pragma unroll
    for (int i = 0; i < CPT; i++) {
        const int y = min(a.y0 + ty * TS + wave + 4 * i, a.y1 - 1);
        area[i] = a.dxc[y] * a.dyc[y];                               // cellArea = dxc * dyc
        const float root = sqrtf(1 + sv[i] * sv[i]);                 // a float sum and the float square root, as the reference compiles
        bedt[i] = area[i] * root;
        zeroish[i] = fabs(hv[i] - 0.0) < 0.000001;
    }
    size_t rec = toff[blockIdx.x];
    for (int prev = -1;; rec++) {
        const int cur = next_index(ci, prev, sm);
        if (cur == NONE) break;
        prev = cur;
        unsigned mine = 0u;
#pragma unroll
        for (int i = 0; i < CPT; i++) if (ci[i] == cur) mine |= 1u << i;
        const bool wave_has = __ballot(mine != 0u) != 0ull;
        if (first) {
            double ca = 0.0;
#pragma unroll
            for (int i = 0; i < CPT; i++) if (mine & (1u << i)) ca += area[i];
            ca = wave_sum(ca);
            if (lane == 0) sArea[wave] = ca;
        }
        if (!wave_has) {
            for (int t = lane; t < 3 * hc; t += 64) sRed[wave][t] = 0.0;
            for (int t = lane; t < hc; t += 64) sCnt[wave][t] = 0;
        } else {
            const unsigned act = mine & wet;
            for (int kk = 0; kk < hc; kk++) {
                const double h = height[k0 + kk];
                int cnt = 0;
                double sa = 0.0, ba = 0.0, vol = 0.0;
#pragma unroll
                for (int i = 0; i < CPT; i++) {
                    if ((act & (1u << i)) && (hv[i] < h || zeroish[i])) {
                        cnt += 1;
                        sa += area[i];
                        ba += bedt[i];
                        vol += (h - hv[i]) * area[i];
                    }
                }
                cnt = wave_sum(cnt); sa = wave_sum(sa); ba = wave_sum(ba); vol = wave_sum(vol);
                if (lane == 0) { sCnt[wave][kk] = cnt; sRed[wave][kk] = sa; sRed[wave][hc + kk] = ba; sRed[wave][2 * hc + kk] = vol; }
            }
        }
        __syncthreads();
        for (int t = threadIdx.x; t < 3 * hc; t += 256) slab[rec * size_t(3 * hc) + t] = ((sRed[0][t] + sRed[1][t]) + sRed[2][t]) + sRed[3][t];
        for (int t = threadIdx.x; t < hc; t += 256) {
            const int c = sCnt[0][t] + sCnt[1][t] + sCnt[2][t] + sCnt[3][t];
            if (c) atomicAdd(&count[size_t(k0 + t) * size_t(ncatch) + size_t(cur)], c);
        }
        if (first && threadIdx.x == 255) {
            areaslab[rec] = ((sArea[0] + sArea[1]) + sArea[2]) + sArea[3];
            keys[rec] = uint32_t(cur);
            vals[rec] = uint32_t(rec);
        }
        __syncthreads();
    }
}

// One workgroup per catchment: its records (a run of the sorted keys) are added in ascending record = ascending tile order.
__global__ __launch_bounds__(256) void chg_reduce_kernel(const uint32_t* __restrict__ skeys, const uint32_t* __restrict__ svals, uint32_t nrec, const double* __restrict__ slab,
                                                         const double* __restrict__ areaslab, int k0, int hc, int ncatch, int first, double* __restrict__ surface,
                                                         double* __restrict__ bed, double* __restrict__ volume, double* __restrict__ catcharea) {
    __shared__ uint32_t range[2];
    const uint32_t c = blockIdx.x;
    if (threadIdx.x < 2) {   // lower bound of c and of c + 1
        const uint64_t want = uint64_t(c) + threadIdx.x;
        uint32_t lo = 0, hi = nrec;
        while (lo < hi) {
            const uint32_t m = lo + (hi - lo) / 2;
            if (uint64_t(skeys[m]) < want) lo = m + 1; else hi = m;
        }
        range[threadIdx.x] = lo;
    }
    __syncthreads();
    const uint32_t lo = range[0], hi = range[1];
    if (lo == hi) return;
    for (int t = threadIdx.x; t < 3 * hc; t += 256) {
        double s = 0.0;
        for (uint32_t r = lo; r < hi; r++) s += slab[size_t(svals[r]) * size_t(3 * hc) + t];
        const int term = t / hc, kk = t - term * hc;
        double* out = term == 0 ? surface : term == 1 ? bed : volume;
        out[size_t(k0 + kk) * size_t(ncatch) + c] = s;
    }
    if (first && threadIdx.x == 255) {
        double s = 0.0;
        for (uint32_t r = lo; r < hi; r++) s += areaslab[svals[r]];
        catcharea[c] = s;
    }
}

// The depth raster (src/InunDepth.cpp:449-473): a cell with data in catch and hand, unmasked (no mask, or a nodata mask cell), whose id has a forecast depth
// hfc >= 0, is written where hfc > hand + 0.001 in double.  With a mask the reference's line 465 skips every cell that got this far.
__global__ __launch_bounds__(256) void inun_map_kernel(const float* __restrict__ hand, const int32_t* __restrict__ cat, const int16_t* __restrict__ mask, size_t first, size_t n,
                                                       float hand_nd, int32_t cat_nd, int16_t mask_nd, Lookup L, const float* __restrict__ depth, float* __restrict__ map) {
    const size_t i = first + size_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= first + n) return;
    float out = -3.0e38f;
    const int32_t id = cat[i];
    const float hv = hand[i];
    const bool masked = mask && mask[i] != mask_nd;
    if (id != cat_nd && !is_nodata_f(hv, hand_nd) && !masked) {
        const int ix = L.find(id);
        if (ix >= 0) {
            const double hfc = depth[ix];
            if (!(hfc < 0.0) && !mask && hfc > hv + 0.001) out = float(hfc - double(hv));
        }
    }
    map[i] = out;
}

template <class T>
T* upload(tdx_context* ctx, int slot, const T* host, size_t n, size_t offset_bytes = 0, size_t total_bytes = 0) {
    char* p = static_cast<char*>(ctx->scratch(slot, std::max(total_bytes, offset_bytes + std::max<size_t>(n, 1) * sizeof(T))));
    if (!p) return nullptr;
    if (n && hipMemcpyAsync(p + offset_bytes, host, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return nullptr;
    return reinterpret_cast<T*>(p + offset_bytes);
}
size_t pad(size_t b) { return (b + 255) & ~size_t(255); }

// sorted distinct ids with the winning (last) row, uploaded into `slot`
bool make_lookup(tdx_context* ctx, int slot, const int32_t* ids, int64_t n, Lookup& L) {
    std::vector<int32_t> order(static_cast<size_t>(n)), keys, win;
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return ids[a] < ids[b]; });
    for (size_t i = 0; i < order.size(); i++) {
        if (!keys.empty() && keys.back() == ids[order[i]]) win.back() = order[i];   // equal ids stay in list order: the last one wins
        else { keys.push_back(ids[order[i]]); win.push_back(order[i]); }
    }
    const size_t kb = pad(keys.size() * 4);
    const int32_t* dk = upload(ctx, slot, keys.data(), keys.size(), 0, 2 * kb + 256);
    const int32_t* dw = upload(ctx, slot, win.data(), win.size(), kb, 2 * kb + 256);
    if (!dk || !dw) return false;
    L.keys = dk; L.win = dw; L.n = int(keys.size());
    return hipStreamSynchronize(ctx->stream) == hipSuccess;   // the host vectors go out of scope here
}

size_t slab_budget() {
    const char* e = getenv("TDX_CHG_SLAB_MB");
    const double mb = e ? atof(e) : 1024.0;
    return size_t(std::max(mb, 0.001) * 1048576.0);
}

// The keyed reduction over the owned rows of a strip.  INUN: depth != nullptr, nh = 0, only `carea` (the wet area per forecast row) is produced.
// Outputs are HOST arrays: count / surface / bed / volume [nh][ncatch], carea [ncatch].
template <bool INUN>
int keyed_impl(tdx_context* ctx, const Strip& st, const char* stage, const float* d_hand, const int32_t* d_cat, const float* d_slp, float hand_nd, int32_t cat_nd, float slp_nd,
               const double* dxc, const double* dyc, const int32_t* ids, int64_t ncatch, const float* depth, const double* stages, int64_t nh, int32_t* count,
               double* surface, double* bed, double* volume, double* carea, tdx_stats* stats, bool own_call = true) {
    TDX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int tiles_x = (st.nx + TS - 1) / TS, tiles_y = (st.y1 - st.y0 + TS - 1) / TS;
    const size_t ntiles = size_t(tiles_x) * size_t(tiles_y);
    const size_t nt = size_t(nh) * size_t(ncatch);
    if (own_call) { ctx->begin_call(stats); strip_mark(ctx, st, stage); }
    TileArgs a{};
    a.hand = d_hand; a.cat = d_cat; a.slp = d_slp; a.nx = st.nx; a.y0 = st.y0; a.y1 = st.y1; a.tiles_x = tiles_x;
    a.hand_nd = hand_nd; a.slp_nd = slp_nd; a.cat_nd = cat_nd;
    if (!make_lookup(ctx, TDX_S_A, ids, ncatch, a.L)) return tdx_fail(ctx, TDX_ERR_NOMEM, "handtools: id lookup");
    const size_t rows = size_t(st.ny_arr), rb = pad(rows * 8), hb = pad(size_t(nh) * 8), db = pad(size_t(ncatch) * 4);
    const size_t small = 2 * rb + hb + db + 256;
    a.dxc = upload(ctx, TDX_S_B, dxc, rows, 0, small);
    a.dyc = upload(ctx, TDX_S_B, dyc, rows, rb, small);
    const double* d_height = upload(ctx, TDX_S_B, stages, size_t(nh), 2 * rb, small);
    if (INUN) a.depth = upload(ctx, TDX_S_B, depth, size_t(ncatch), 2 * rb + hb, small);
    if (!a.dxc || !a.dyc || !d_height || (INUN && !a.depth)) return tdx_fail(ctx, TDX_ERR_NOMEM, "handtools: tables");
    // records per tile, numbered in tile order
    uint32_t* d_tcount = static_cast<uint32_t*>(ctx->scratch(TDX_S_C, 2 * pad(ntiles * 4)));
    if (!d_tcount) return TDX_ERR_NOMEM;
    uint32_t* d_toff = d_tcount + pad(ntiles * 4) / 4;
    std::vector<uint32_t> tc(ntiles);
    {
        TdxSpan sp(ctx, TDX_K_MISC);
        hipLaunchKernelGGL(chg_count_kernel<INUN>, dim3(unsigned(ntiles)), dim3(256), 0, s, a, d_tcount);
    }
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(tc.data(), d_tcount, ntiles * 4, hipMemcpyDeviceToHost, s));
    TDX_HIP_CHECK(ctx, hipStreamSynchronize(s));
    uint64_t nrec64 = 0;
    uint32_t most = 0;
    for (size_t t = 0; t < ntiles; t++) { const uint32_t n = tc[t]; tc[t] = uint32_t(nrec64); nrec64 += n; most = std::max(most, n); }
    if (nrec64 > 0xfffffff0ull) return tdx_fail(ctx, TDX_ERR_ARG, "handtools: more than 2^32 (tile, catchment) records in one strip");
    const size_t nrec = size_t(nrec64);
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(d_toff, tc.data(), ntiles * 4, hipMemcpyHostToDevice, s));
    // outputs on the device: count | surface | bed | volume | carea
    const size_t ob = pad(nt * 8), cb = pad(nt * 4), ab = pad(size_t(ncatch) * 8);
    char* d_out = static_cast<char*>(ctx->scratch(TDX_S_H, cb + 3 * ob + ab));
    if (!d_out) return TDX_ERR_NOMEM;
    TDX_HIP_CHECK(ctx, hipMemsetAsync(d_out, 0, cb + 3 * ob + ab, s));
    int32_t* d_count = reinterpret_cast<int32_t*>(d_out);
    double *d_surf = reinterpret_cast<double*>(d_out + cb), *d_bed = reinterpret_cast<double*>(d_out + cb + ob), *d_vol = reinterpret_cast<double*>(d_out + cb + 2 * ob);
    double* d_carea = reinterpret_cast<double*>(d_out + cb + 3 * ob);
    int64_t chunks = 0;
    size_t slab_bytes = 0;
    if (nrec > 0) {
        int hc = int(std::min<int64_t>(nh, HC_MAX));
        if (hc > 0) hc = int(std::max<size_t>(1, std::min<size_t>(size_t(hc), slab_budget() / (nrec * 24))));
        slab_bytes = nrec * size_t(std::max(hc, 1)) * 24;
        double* d_slab = static_cast<double*>(ctx->scratch(TDX_S_D, slab_bytes));
        double* d_areaslab = static_cast<double*>(ctx->scratch(TDX_S_E, nrec * 8));
        uint32_t* d_kv = static_cast<uint32_t*>(ctx->scratch(TDX_S_F, 4 * pad(nrec * 4)));
        if (!d_slab || !d_areaslab || !d_kv) return TDX_ERR_NOMEM;
        const size_t kw = pad(nrec * 4) / 4;
        uint32_t *d_keys = d_kv, *d_vals = d_kv + kw, *d_skeys = d_kv + 2 * kw, *d_svals = d_kv + 3 * kw;
        TdxSpan sp(ctx, TDX_K_ACCUM);
        for (int64_t k0 = 0; k0 == 0 || k0 < nh; k0 += std::max(hc, 1)) {
            const int h = int(std::min<int64_t>(hc, nh - k0)), first = k0 == 0;
            hipLaunchKernelGGL(chg_tile_kernel<INUN>, dim3(unsigned(ntiles)), dim3(256), 0, s, a, d_toff, d_height, int(k0), h, int(ncatch), first, d_slab, d_areaslab, d_keys,
                               d_vals, d_count);
            if (first) {
                const int rc = tdx_sort_pairs_u32(ctx, TDX_S_G, d_keys, d_skeys, d_vals, d_svals, nrec);
                if (rc != TDX_OK) return rc;
            }
            hipLaunchKernelGGL(chg_reduce_kernel, dim3(unsigned(ncatch)), dim3(256), 0, s, d_skeys, d_svals, uint32_t(nrec), d_slab, d_areaslab, int(k0), h, int(ncatch), first,
                               d_surf, d_bed, d_vol, d_carea);
            chunks++;
        }
        if (stats) stats->launches[TDX_K_ACCUM] += 2 * chunks;
    }
    TDX_HIP_CHECK(ctx, hipGetLastError());
    if (nt) {
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(count, d_count, nt * 4, hipMemcpyDeviceToHost, s));
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(surface, d_surf, nt * 8, hipMemcpyDeviceToHost, s));
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(bed, d_bed, nt * 8, hipMemcpyDeviceToHost, s));
        TDX_HIP_CHECK(ctx, hipMemcpyAsync(volume, d_vol, nt * 8, hipMemcpyDeviceToHost, s));
    }
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(carea, d_carea, size_t(ncatch) * 8, hipMemcpyDeviceToHost, s));
    tdx_stats* stt = stats;
    if (own_call) ctx->end_call(); else TDX_HIP_CHECK(ctx, hipStreamSynchronize(s));
    // rounds: stage chunks; cells_evaluated: (tile, catchment) records; levels_fall_max: the most records of one tile; flats_initial: slab bytes
    if (stt) { stt->rounds = chunks; stt->cells_evaluated = int64_t(nrec); stt->levels_fall_max = most; stt->flats_initial = int64_t(slab_bytes); }
    return TDX_OK;
}

int inun_impl(tdx_context* ctx, const Strip& st, const float* d_hand, const int32_t* d_cat, const int16_t* d_mask, float hand_nd, int32_t cat_nd, int16_t mask_nd,
              const double* dxc, const double* dyc, const int32_t* ids, const float* depth, int64_t nfc, float* d_map, double* area, tdx_stats* stats) {
    TDX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    ctx->begin_call(stats);
    strip_mark(ctx, st, "inundepth");
    if (area) {   // first: it leaves the lookup and the depths where the map kernel wants them
        const int rc = keyed_impl<true>(ctx, st, "inundepth", d_hand, d_cat, nullptr, hand_nd, cat_nd, 0.f, dxc, dyc, ids, nfc, depth, nullptr, 0, nullptr, nullptr, nullptr, nullptr,
                                        area, stats, false);
        if (rc != TDX_OK) return rc;
    }
    Lookup L{};
    if (!make_lookup(ctx, TDX_S_A, ids, nfc, L)) return tdx_fail(ctx, TDX_ERR_NOMEM, "inundepth: id lookup");
    const float* d_depth = upload(ctx, TDX_S_I, depth, size_t(nfc));
    if (!d_depth) return tdx_fail(ctx, TDX_ERR_NOMEM, "inundepth: depths");
    const size_t first = size_t(st.y0) * size_t(st.nx), nown = size_t(st.y1 - st.y0) * size_t(st.nx);
    {
        TdxSpan sp(ctx, TDX_K_STENCIL);
        hipLaunchKernelGGL(inun_map_kernel, dim3(tdx_blocks_for(nown, 256)), dim3(256), 0, s, d_hand, d_cat, d_mask, first, nown, hand_nd, cat_nd, mask_nd, L, d_depth, d_map);
        if (stats) stats->launches[TDX_K_STENCIL] += 1;
    }
    TDX_HIP_CHECK(ctx, hipGetLastError());
    ctx->end_call();
    return TDX_OK;
}

bool bad_tables(int64_t ncatch, int64_t nh) { return ncatch <= 0 || ncatch > 0x7ffffff0 || nh < 0 || nh > 0x7ffffff0 || uint64_t(ncatch) * uint64_t(std::max<int64_t>(nh, 1)) > 0x7ffffff0ull; }

}  // namespace

extern "C" int tdx_catchhydrogeo_dev(tdx_context* ctx, const float* d_hand, const int32_t* d_catch, const float* d_slp, int64_t nx, int64_t ny, float hand_nodata,
                                     int32_t catch_nodata, float slp_nodata, const double* dxc, const double* dyc, const int32_t* ids, int64_t ncatch, const double* stages,
                                     int64_t nheight, int32_t* count, double* surface, double* bed, double* volume, double* catcharea, tdx_stats* stats) {
    if (!ctx || !d_hand || !d_catch || !d_slp || !dxc || !dyc || !ids || !catcharea || nx <= 0 || ny <= 0 || (nheight > 0 && (!stages || !count || !surface || !bed || !volume)))
        return tdx_fail(ctx, TDX_ERR_ARG, "tdx_catchhydrogeo_dev: bad argument");
    if (bad_tables(ncatch, nheight)) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_catchhydrogeo_dev: the table nheight x ncatch needs 1 .. 2^31 entries");
    if (too_big(nx, ny)) return tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip");
    return keyed_impl<false>(ctx, strip_single(int(nx), int(ny)), "catchhydrogeo", d_hand, d_catch, d_slp, hand_nodata, catch_nodata, slp_nodata, dxc, dyc, ids, ncatch, nullptr, stages,
                             nheight, count, surface, bed, volume, catcharea, stats);
}
extern "C" int tdx_catchhydrogeo_strip(tdx_context* ctx, const tdx_comm* comm, const float* d_hand, const int32_t* d_catch, const float* d_slp, int64_t nx, int64_t ny_local,
                                       float hand_nodata, int32_t catch_nodata, float slp_nodata, const double* dxc, const double* dyc, const int32_t* ids, int64_t ncatch,
                                       const double* stages, int64_t nheight, int32_t* count, double* surface, double* bed, double* volume, double* catcharea, tdx_stats* stats) {
    if (!ctx || !d_hand || !d_catch || !d_slp || !dxc || !dyc || !ids || !catcharea || nx <= 0 || ny_local <= 0 ||
        (nheight > 0 && (!stages || !count || !surface || !bed || !volume)))
        return tdx_fail(ctx, TDX_ERR_ARG, "tdx_catchhydrogeo_strip: bad argument");
    if (bad_tables(ncatch, nheight)) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_catchhydrogeo_strip: the table nheight x ncatch needs 1 .. 2^31 entries");
    if (too_big(nx, ny_local + 2)) return tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip");
    return keyed_impl<false>(ctx, strip_from_comm(comm, int(nx), int(ny_local)), "catchhydrogeo", d_hand, d_catch, d_slp, hand_nodata, catch_nodata, slp_nodata, dxc, dyc, ids, ncatch,
                             nullptr, stages, nheight, count, surface, bed, volume, catcharea, stats);
}
extern "C" int tdx_catchhydrogeo(tdx_context* ctx, const float* hand, const int32_t* catchr, const float* slp, int64_t nx, int64_t ny, float hand_nodata, int32_t catch_nodata,
                                 float slp_nodata, const double* dxc, const double* dyc, const int32_t* ids, int64_t ncatch, const double* stages, int64_t nheight, int32_t* count,
                                 double* surface, double* bed, double* volume, double* catcharea, tdx_stats* stats) {
    if (!ctx || !hand || !catchr || !slp || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_catchhydrogeo: bad argument");
    HostCall h(ctx, nx, ny);   // no raster comes back: the tables are host arrays, written by the _dev form
    float* d_h = h.in(TDX_S_IO0, hand);
    int32_t* d_c = h.in(TDX_S_IO1, catchr);
    float* d_s = h.in(TDX_S_IO2, slp);
    if (h.error) return h.error;
    return h.finish(tdx_catchhydrogeo_dev(ctx, d_h, d_c, d_s, nx, ny, hand_nodata, catch_nodata, slp_nodata, dxc, dyc, ids, ncatch, stages, nheight, count, surface, bed, volume,
                                          catcharea, stats));
}

extern "C" int tdx_inundepth_strip(tdx_context* ctx, const tdx_comm* comm, const float* d_hand, const int32_t* d_catch, const int16_t* d_mask, int64_t nx, int64_t ny_local,
                                   float hand_nodata, int32_t catch_nodata, int16_t mask_nodata, const double* dxc, const double* dyc, const int32_t* ids, const float* depth,
                                   int64_t nfc, float* d_map, double* area_partial, tdx_stats* stats) {
    if (!ctx || !d_hand || !d_catch || !d_map || !ids || !depth || nx <= 0 || ny_local <= 0 || (area_partial && (!dxc || !dyc)))
        return tdx_fail(ctx, TDX_ERR_ARG, "tdx_inundepth_strip: bad argument");
    if (bad_tables(nfc, 0)) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_inundepth_strip: 1 .. 2^31 forecast rows");
    if (too_big(nx, ny_local + 2)) return tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip");
    return inun_impl(ctx, strip_from_comm(comm, int(nx), int(ny_local)), d_hand, d_catch, d_mask, hand_nodata, catch_nodata, mask_nodata, dxc, dyc, ids, depth, nfc, d_map,
                     area_partial, stats);
}
extern "C" int tdx_inundepth_dev(tdx_context* ctx, const float* d_hand, const int32_t* d_catch, const int16_t* d_mask, int64_t nx, int64_t ny, float hand_nodata,
                                 int32_t catch_nodata, int16_t mask_nodata, const double* dxc, const double* dyc, const int32_t* ids, const float* depth, int64_t nfc, float* d_map,
                                 float* area, tdx_stats* stats) {
    if (!ctx || !d_hand || !d_catch || !d_map || !ids || !depth || nx <= 0 || ny <= 0 || (area && (!dxc || !dyc))) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_inundepth_dev: bad argument");
    if (bad_tables(nfc, 0)) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_inundepth_dev: 1 .. 2^31 forecast rows");
    if (too_big(nx, ny)) return tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip");
    std::vector<double> wide(area ? size_t(nfc) : 0);
    const int rc = inun_impl(ctx, strip_single(int(nx), int(ny)), d_hand, d_catch, d_mask, hand_nodata, catch_nodata, mask_nodata, dxc, dyc, ids, depth, nfc, d_map,
                             area ? wide.data() : nullptr, stats);
    if (rc == TDX_OK && area) for (size_t i = 0; i < wide.size(); i++) area[i] = float(wide[i]);   // fp64 sum, rounded once
    return rc;
}
extern "C" int tdx_inundepth(tdx_context* ctx, const float* hand, const int32_t* catchr, const int16_t* mask, int64_t nx, int64_t ny, float hand_nodata, int32_t catch_nodata,
                             int16_t mask_nodata, const double* dxc, const double* dyc, const int32_t* ids, const float* depth, int64_t nfc, float* map, float* area,
                             tdx_stats* stats) {
    if (!ctx || !hand || !catchr || !map || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_inundepth: bad argument");
    HostCall h(ctx, nx, ny);
    float* d_h = h.in(TDX_S_IO0, hand);
    int32_t* d_c = h.in(TDX_S_IO1, catchr);
    float* d_o = h.out(TDX_S_IO2, map);
    int16_t* d_m = h.in(TDX_S_IO3, mask);   // optional
    if (h.error) return h.error;
    return h.finish(tdx_inundepth_dev(ctx, d_h, d_c, d_m, nx, ny, hand_nodata, catch_nodata, mask_nodata, dxc, dyc, ids, depth, nfc, d_o, area, stats));
}
