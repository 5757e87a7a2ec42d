// MoveOutletsToStrm and ConnectDown: outlets onto streams.
//   tdx_moveoutlets*   <- the walk of outletstosrc()  src/MoveOutletsToStrm.cpp:370-435
//   tdx_connectdown*   <- connectdown()               src/ConnectDown.cpp:177-247 (maximum of each watershed), :402-434 (the walk)
//
// The walk: one lane per point on rasters that stay in device memory; a pipeline that holds p and src (or w) on the device moves its few hundred
// points without a download of 2-6 bytes per cell.  A strip advances the points in its owned rows and hands the state back (global rows).
//
// The maximum of each watershed: one streaming pass over w and ad8 (8 bytes per cell).  Every lane reads ARG_CELLS consecutive cells with 16-byte
// loads and merges them in registers; lanes that hold one id merge with their neighbours of the same id through a segmented scan of lane shuffles;
// the last lane of every run issues ONE 64-bit atomic max (agent scope, no return value) into table[id].  A lane whose cells hold several ids issues
// one atomic per run of its own: checkerboard ids cost one atomic per cell and stay correct.  The key orders (value, then the SMALLER cell index):
//   high word  the float mapped order-preserving to unsigned, -0.0 as +0.0, every NaN as 0 (below -inf, which maps to 0x007fffff);
//   low word   the complement of the cell's index in the array (< 2^32 - 1, so that no key is 0: 0 is "id not present").
// The reference starts from the id's FIRST cell and replaces it with a strict >: a NaN there is never replaced.  So when the pass has met a NaN at
// all (a flag), a second pass takes the minimum cell index of every id, and the decode step picks that cell where it holds a NaN.  Rasters
// without NaN never run it.  A strip reports both - its maximum over the cells that are not NaN, and its first cell where that holds a NaN - because
// only the first strip that holds the id may let the NaN stand (tdx_connectdown_merge).
#include <algorithm>
#include <cstring>
#include <vector>

#include "context.hpp"
#include "device_common.hpp"
#include "strips.hpp"

struct tdx_connectdown_points {
    std::vector<int32_t> ids, x, y, mx, my, id_down;   // y / my: rows of the whole raster
    std::vector<float> ad8max;
    // a strip's part only: where the FIRST cell of the id in the strip holds a NaN, that cell (x / y / ad8max are then the maximum of the cells that
    // do not, as everywhere; of an id with nothing but NaN the first cell again)
    std::vector<int32_t> first_x, first_y;
    std::vector<float> first_val;
    std::vector<uint8_t> first_is_nan;
    double phase_ms[TDX_CONNECTDOWN_PHASES] = {0, 0, 0, 0};
};

namespace {
using namespace tdxk;

// ---------------------------------------------------------------------------------------------------------------- the walk
enum { WALK_MOVEOUTLETS = 0, WALK_CONNECTDOWN = 1 };

// Arrays of arr_rows rows whose row 0 is row arr_row0 of a raster of ny_total rows; the lane owns a point while its row is in [own0, own1) (global).
// state: x, y (global row), dist, done.  side: src (MoveOutlets) or w (ConnectDown).  moved: points this launch advanced or finished.
template <int POLICY>
__global__ __launch_bounds__(256) void walk_kernel(const int16_t* __restrict__ P, const int32_t* __restrict__ side, int nx, int ny_total, int arr_row0, int own0, int own1,
                                                   int16_t p_nodata, int32_t side_nodata, int limit, int32_t* __restrict__ sx, int32_t* __restrict__ sy,
                                                   int32_t* __restrict__ sdist, int32_t* __restrict__ sdone, int32_t* __restrict__ iddown, unsigned npts,
                                                   unsigned long long* __restrict__ moved) {
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    bool touched = false;
    if (i < npts && !sdone[i]) {
        int x = sx[i], y = sy[i], dist = sdist[i];
        bool done = false;
        int32_t down = 0;
        bool have_down = false;
        if (x < 0 || x >= nx || y < 0 || y >= ny_total) {   // off the raster: cannot be moved (src/MoveOutletsToStrm.cpp:375-378)
            done = true; dist = -1; touched = true;
        }
        while (!done && y >= own0 && y < own1) {
            touched = true;
            const size_t c = size_t(y - arr_row0) * size_t(nx) + size_t(x);
            const int16_t p = P[c];
            const int32_t s = side[c];
            bool step;
            if (POLICY == WALK_MOVEOUTLETS) {
                if (p == p_nodata) done = true;                       // :390-392: done, and the body below still runs once
                step = (s == side_nodata) || s < 1;                   // :397 not on the stream
                if (!step) done = true;                               // :427-429
            } else {
                down = s; have_down = true;                           // src/ConnectDown.cpp:413
                step = true;
            }
            if (step) {
                if (p >= 1 && p <= 8 && dist < limit) {
                    const int xn = x + d1(p), yn = y + d2(p);
                    if (xn >= 0 && yn >= 0 && xn < nx && yn < ny_total) { x = xn; y = yn; dist++; }
                    else { done = true; if (POLICY == WALK_MOVEOUTLETS) dist = -1; }   // moved off the map
                } else {
                    done = true; if (POLICY == WALK_MOVEOUTLETS) dist = -1;            // not a direction, or maxdist steps walked
                }
            }
        }
        if (touched) {
            sx[i] = x; sy[i] = y; sdist[i] = dist; sdone[i] = done ? 1 : 0;
            if (POLICY == WALK_CONNECTDOWN && have_down && done) iddown[i] = down;
        }
    }
    const unsigned long long b = __ballot(touched);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(moved, (unsigned long long)__popcll(b));
}

// State on the host in and out; the rasters are device arrays of (own1 - own0) rows (+ 2 halo rows when halo).
int walk_run(tdx_context* ctx, int policy, const int16_t* d_p, const int32_t* d_side, int nx, int ny_total, int arr_row0, int own0, int own1, int16_t p_nodata,
             int32_t side_nodata, int limit, int32_t* sx, int32_t* sy, int32_t* sdist, int32_t* sdone, int32_t* iddown, int64_t npts, int64_t* n_moved) {
    if (n_moved) *n_moved = 0;
    if (npts == 0) return TDX_OK;
    hipStream_t s = ctx->stream;
    const size_t n = size_t(npts), nb = n * 4;
    int32_t* buf = static_cast<int32_t*>(ctx->scratch(TDX_S_K, 5 * nb + 16));
    if (!buf) return tdx_fail(ctx, TDX_ERR_NOMEM, "outlet walk: out of device memory");
    int32_t *dx = buf, *dy = buf + n, *dd = buf + 2 * n, *dn = buf + 3 * n, *di = buf + 4 * n;
    unsigned long long* d_moved = reinterpret_cast<unsigned long long*>(ctx->d_mail + TDX_MAIL_STAGE);
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(dx, sx, nb, hipMemcpyHostToDevice, s));
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(dy, sy, nb, hipMemcpyHostToDevice, s));
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(dd, sdist, nb, hipMemcpyHostToDevice, s));
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(dn, sdone, nb, hipMemcpyHostToDevice, s));
    if (iddown) TDX_HIP_CHECK(ctx, hipMemcpyAsync(di, iddown, nb, hipMemcpyHostToDevice, s));
    TDX_HIP_CHECK(ctx, hipMemsetAsync(d_moved, 0, 8, s));
    const dim3 grid(tdx_blocks_for(n, 256));
    if (policy == WALK_MOVEOUTLETS)
        hipLaunchKernelGGL(walk_kernel<WALK_MOVEOUTLETS>, grid, dim3(256), 0, s, d_p, d_side, nx, ny_total, arr_row0, own0, own1, p_nodata, side_nodata, limit, dx, dy, dd, dn,
                           di, unsigned(n), d_moved);
    else
        hipLaunchKernelGGL(walk_kernel<WALK_CONNECTDOWN>, grid, dim3(256), 0, s, d_p, d_side, nx, ny_total, arr_row0, own0, own1, p_nodata, side_nodata, limit, dx, dy, dd, dn,
                           di, unsigned(n), d_moved);
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(sx, dx, nb, hipMemcpyDeviceToHost, s));
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(sy, dy, nb, hipMemcpyDeviceToHost, s));
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(sdist, dd, nb, hipMemcpyDeviceToHost, s));
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(sdone, dn, nb, hipMemcpyDeviceToHost, s));
    if (iddown) TDX_HIP_CHECK(ctx, hipMemcpyAsync(iddown, di, nb, hipMemcpyDeviceToHost, s));
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(ctx->h_mail + TDX_MAIL_STAGE, d_moved, 8, hipMemcpyDeviceToHost, s));
    TDX_HIP_CHECK(ctx, hipStreamSynchronize(s));
    if (n_moved) *n_moved = int64_t(ctx->h_mail[TDX_MAIL_STAGE]);
    return TDX_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the maximum of each watershed
constexpr int ARG_CELLS = 8, ARG_BLOCK_CELLS = 256 * ARG_CELLS;

__device__ __forceinline__ uint32_t order_word(float v) {
    if (v != v) return 0u;
    uint32_t u = __builtin_bit_cast(uint32_t, v);
    if (u == 0x80000000u) u = 0u;   // -0.0 ties with +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ unsigned long long arg_key(float v, uint32_t index) { return ((unsigned long long)order_word(v) << 32) | (unsigned long long)(~index); }
__device__ __forceinline__ void table_max(unsigned long long* __restrict__ table, int32_t id, unsigned long long key) {
    (void)__hip_atomic_fetch_max(table + size_t(uint32_t(id)), key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long shfl_up_u64(unsigned long long v, int off) {
    const uint32_t lo = __shfl_up(uint32_t(v), off, 64), hi = __shfl_up(uint32_t(v >> 32), off, 64);
    return ((unsigned long long)hi << 32) | lo;
}

// the ARG_CELLS cells of a lane: 16-byte loads where the lane's span lies inside [first, first + count) and is 16-byte aligned (vec: the same answer for
// every lane of the launch, their spans are 32 bytes apart), single loads otherwise; a cell past the end is nodata
__device__ __forceinline__ void load_cells(const int32_t* __restrict__ W, const float* __restrict__ A, size_t base, size_t end, bool vec, int32_t nodata,
                                           int32_t (&w)[ARG_CELLS], float (&a)[ARG_CELLS]) {
    if (vec && base + ARG_CELLS <= end) {
        const int4 w0 = *reinterpret_cast<const int4*>(W + base), w1 = *reinterpret_cast<const int4*>(W + base + 4);
        w[0] = w0.x; w[1] = w0.y; w[2] = w0.z; w[3] = w0.w; w[4] = w1.x; w[5] = w1.y; w[6] = w1.z; w[7] = w1.w;
        if (A) {
            const float4 a0 = *reinterpret_cast<const float4*>(A + base), a1 = *reinterpret_cast<const float4*>(A + base + 4);
            a[0] = a0.x; a[1] = a0.y; a[2] = a0.z; a[3] = a0.w; a[4] = a1.x; a[5] = a1.y; a[6] = a1.z; a[7] = a1.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < ARG_CELLS; i++) {
            const size_t c = base + size_t(i);
            w[i] = c < end ? W[c] : nodata;
            if (A) a[i] = c < end ? A[c] : 0.f;
        }
    }
}

// largest and smallest id (as id ^ 0x80000000, unsigned) of the cells [first, first + count): mm[0] max (starts at 0), mm[1] min (starts at ~0)
__global__ __launch_bounds__(256) void id_range_kernel(const int32_t* __restrict__ W, size_t first, size_t count, bool vec, int32_t nodata, uint32_t* __restrict__ mm) {
    const size_t end = first + count;
    uint32_t hi = 0u, lo = 0xffffffffu;
    for (size_t base = first + (size_t(blockIdx.x) * 256 + threadIdx.x) * ARG_CELLS; base < end; base += size_t(gridDim.x) * ARG_BLOCK_CELLS) {
        int32_t w[ARG_CELLS];
        float unused[ARG_CELLS];
        load_cells(W, nullptr, base, end, vec, nodata, w, unused);
#pragma unroll
        for (int i = 0; i < ARG_CELLS; i++)
            if (w[i] != nodata) { const uint32_t u = uint32_t(w[i]) ^ 0x80000000u; hi = max(hi, u); lo = min(lo, u); }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { hi = max(hi, uint32_t(__shfl_down(hi, off, 64))); lo = min(lo, uint32_t(__shfl_down(lo, off, 64))); }
    if ((threadIdx.x & 63) == 0) {
        if (hi != 0u) atomicMax(mm, hi);
        if (lo != 0xffffffffu) atomicMin(mm + 1, lo);
    }
}

// FIRST == false: table[id] = max key over the id's cells; *nan_flag raised when a NaN was met.  FIRST == true: first_cell[id] = min cell index.
// Cell indices count from the start of the array (index_of(first) = first).
template <bool FIRST>
__global__ __launch_bounds__(256) void argmax_kernel(const int32_t* __restrict__ W, const float* __restrict__ A, size_t first, size_t count, bool vec, int32_t nodata,
                                                     unsigned long long* __restrict__ table, uint32_t* __restrict__ first_cell, uint32_t* __restrict__ nan_flag) {
    const size_t end = first + count;
    const size_t base = first + (size_t(blockIdx.x) * 256 + threadIdx.x) * ARG_CELLS;   // (past the end for the last lanes: they hold no cell and still shuffle)
    const int lane = int(threadIdx.x & 63);
    int32_t w[ARG_CELLS];
    float a[ARG_CELLS];
    if (base < end) load_cells(W, FIRST ? nullptr : A, base, end, vec, nodata, w, a);
    else {
#pragma unroll
        for (int i = 0; i < ARG_CELLS; i++) { w[i] = nodata; a[i] = 0.f; }
    }
    // runs of this lane: nodata cells are skipped, a run ends where the id changes
    bool have = false, single = true, saw_nan = false;
    int32_t id = 0;
    unsigned long long key = 0;
#pragma unroll
    for (int i = 0; i < ARG_CELLS; i++) {
        if (w[i] == nodata) continue;
        const uint32_t idx = uint32_t(base + size_t(i));
        unsigned long long k;
        if (FIRST) k = (unsigned long long)(~idx);
        else { k = arg_key(a[i], idx); saw_nan |= a[i] != a[i]; }
        if (have && w[i] != id) {   // the run before this cell is complete and the lane holds several ids: it goes out on its own
            single = false;
            if (FIRST) atomicMin(first_cell + size_t(uint32_t(id)), ~uint32_t(key)); else table_max(table, id, key);
            key = 0;
        }
        have = true; id = w[i];
        key = max(key, k);
    }
    if (have && !single) {          // the last run of a lane with several ids
        if (FIRST) atomicMin(first_cell + size_t(uint32_t(id)), ~uint32_t(key)); else table_max(table, id, key);
    }
    const bool whole = have && single;   // the lane's cells are one run: merge it with the neighbouring lanes of the same id
    const int32_t prev_id = __shfl_up(id, 1, 64);
    const int prev_whole = __shfl_up(int(whole), 1, 64);
    const bool head = !whole || lane == 0 || !prev_whole || prev_id != id;
    const unsigned long long heads = __ballot(head);
    const int seg = 63 - __clzll((long long)(heads & ((2ull << lane) - 1ull)));   // first lane of this lane's run (bit `lane` is set for a head; lane 0 always is one)
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long t = shfl_up_u64(key, off);
        if (lane - off >= seg) key = max(key, t);
    }
    const bool tail = whole && (lane == 63 || ((heads >> (lane + 1)) & 1ull));
    if (tail) {
        if (FIRST) atomicMin(first_cell + size_t(uint32_t(id)), ~uint32_t(key)); else table_max(table, id, key);
    }
    if (!FIRST && __ballot(saw_nan) && lane == 0) *nan_flag = 1u;
}

// exclusive prefix of `c` over the 256 threads of the block; *total: the block's sum
__device__ __forceinline__ unsigned block_scan256(unsigned c, unsigned* total) {
    __shared__ unsigned s_wave[4];
    const int lane = int(threadIdx.x & 63), wv = int(threadIdx.x >> 6);
    unsigned v = c;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned t = __shfl_up(v, off, 64);
        if (lane >= off) v += t;
    }
    __syncthreads();   // an earlier use of s_wave is over
    if (lane == 63) s_wave[wv] = v;
    __syncthreads();
    unsigned wave_off = 0;
    for (int i = 0; i < wv; i++) wave_off += s_wave[i];
    *total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    return wave_off + (v - c);
}
constexpr int DEC_IDS = 8, DEC_BLOCK_IDS = 256 * DEC_IDS;
__device__ __forceinline__ unsigned present_mask(const unsigned long long* __restrict__ table, size_t base, size_t m) {
    unsigned mask = 0;
#pragma unroll
    for (int i = 0; i < DEC_IDS; i++)
        if (base + size_t(i) < m && table[base + size_t(i)] != 0ull) mask |= 1u << i;
    return mask;
}
__global__ __launch_bounds__(256) void present_count_kernel(const unsigned long long* __restrict__ table, size_t m, uint32_t* __restrict__ block_count) {
    unsigned total;
    block_scan256(unsigned(__popc(present_mask(table, size_t(blockIdx.x) * DEC_BLOCK_IDS + size_t(threadIdx.x) * DEC_IDS, m))), &total);
    if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}
// one block: block_count -> exclusive offsets in place, the sum to *total
__global__ __launch_bounds__(256) void present_offsets_kernel(uint32_t* __restrict__ block_count, unsigned nblocks, unsigned long long* __restrict__ total) {
    __shared__ unsigned s_carry;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (unsigned b0 = 0; b0 < nblocks; b0 += 256) {
        const unsigned b = b0 + threadIdx.x;
        const unsigned c = b < nblocks ? block_count[b] : 0u;
        unsigned chunk;
        const unsigned ex = block_scan256(c, &chunk);
        const unsigned carry = s_carry;
        if (b < nblocks) block_count[b] = carry + ex;
        __syncthreads();
        if (threadIdx.x == 0) s_carry = carry + chunk;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = s_carry;
}
// ids, cells and values of the ids present, in ascending id: the cell of the key, and - with first_cell - the id's first cell where that cell holds a
// NaN (NO_CELL where it does not)
constexpr uint32_t NO_CELL = 0xffffffffu;
__global__ __launch_bounds__(256) void decode_kernel(const unsigned long long* __restrict__ table, size_t m, const uint32_t* __restrict__ block_off,
                                                     const uint32_t* __restrict__ first_cell, const float* __restrict__ A, int32_t* __restrict__ out_id,
                                                     uint32_t* __restrict__ out_cell, float* __restrict__ out_val, uint32_t* __restrict__ out_first,
                                                     float* __restrict__ out_first_val) {
    const size_t base = size_t(blockIdx.x) * DEC_BLOCK_IDS + size_t(threadIdx.x) * DEC_IDS;
    const unsigned mask = present_mask(table, base, m);
    unsigned total;
    unsigned r = block_off[blockIdx.x] + block_scan256(unsigned(__popc(mask)), &total);
#pragma unroll
    for (int i = 0; i < DEC_IDS; i++) {
        if (!((mask >> i) & 1u)) continue;
        const size_t id = base + size_t(i);
        const uint32_t cell = ~uint32_t(table[id]);
        uint32_t first = NO_CELL;
        float fv = 0.f;
        if (first_cell) { const uint32_t f = first_cell[id]; const float v = A[f]; if (v != v) { first = f; fv = v; } }
        out_id[r] = int32_t(id); out_cell[r] = cell; out_val[r] = A[cell]; out_first[r] = first; out_first_val[r] = fv;
        r++;
    }
}

struct PhaseEvents {
    tdx_context* ctx;
    hipEvent_t a[TDX_CONNECTDOWN_PHASES], b[TDX_CONNECTDOWN_PHASES];
    bool used[TDX_CONNECTDOWN_PHASES] = {false, false, false, false};
    explicit PhaseEvents(tdx_context* c) : ctx(c) {}
    void begin(int k) { a[k] = ctx->get_event(); b[k] = ctx->get_event(); used[k] = true; (void)hipEventRecord(a[k], ctx->stream); }
    void end(int k) { (void)hipEventRecord(b[k], ctx->stream); }
    void read(double* ms) {   // after the stream has been drained
        for (int k = 0; k < TDX_CONNECTDOWN_PHASES; k++) {
            float t = 0;
            ms[k] = (used[k] && hipEventElapsedTime(&t, a[k], b[k]) == hipSuccess) ? double(t) : 0.0;
        }
    }
};

// The maxima of the ids in the cells [first, first + count) of the arrays W / A: res->ids, res->ad8max and `cells` (the cell's INDEX in the array, for
// the caller to split into column and row).  st != nullptr: the table is sized by the largest id of ALL strips (an all-reduce).
int argmax_run(tdx_context* ctx, const Strip* st, const int32_t* W, const float* A, size_t first, size_t count, int32_t w_nodata, tdx_connectdown_points* res,
               std::vector<uint32_t>& cells, std::vector<uint32_t>& firsts, PhaseEvents& ev, const char* who) {
    hipStream_t s = ctx->stream;
    const bool vec = ((reinterpret_cast<uintptr_t>(W + first) | reinterpret_cast<uintptr_t>(A + first)) & 15u) == 0;
    uint32_t* mm = reinterpret_cast<uint32_t*>(ctx->d_mail + TDX_MAIL_STAGE);   // words 0, 1: max, min; word 2 (of 4 bytes): the NaN flag
    const uint32_t init[4] = {0u, 0xffffffffu, 0u, 0u};
    const unsigned nblocks = tdx_blocks_for(count, ARG_BLOCK_CELLS);
    ev.begin(TDX_CONNECTDOWN_MAXID);
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(mm, init, sizeof init, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(id_range_kernel, dim3(std::min(nblocks, unsigned(ctx->num_cus) * 8u)), dim3(256), 0, s, W, first, count, vec, w_nodata, mm);
    ev.end(TDX_CONNECTDOWN_MAXID);
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(ctx->h_mail + TDX_MAIL_STAGE, mm, 8, hipMemcpyDeviceToHost, s));
    TDX_HIP_CHECK(ctx, hipStreamSynchronize(s));
    uint32_t h[2];
    memcpy(h, ctx->h_mail + TDX_MAIL_STAGE, 8);
    const bool any = h[0] != 0u || h[1] != 0xffffffffu;
    int64_t lohi[2] = {any ? -int64_t(int32_t(h[1] ^ 0x80000000u)) : int64_t(-0x7fffffff), any ? int64_t(int32_t(h[0] ^ 0x80000000u)) : int64_t(-1)};   // {-min, max}
    if (st) { if (int rc = strip_allreduce(ctx, *st, lohi, 2, TDX_OP_MAX)) return rc; }
    if (lohi[1] < 0 && -lohi[0] > lohi[1]) return TDX_OK;   // no id at all (anywhere)
    if (-lohi[0] < 0) return tdx_fail(ctx, TDX_ERR_ARG, std::string(who) + ": negative watershed id " + std::to_string(-lohi[0]));
    if (lohi[1] > TDX_CONNECTDOWN_MAX_ID)
        return tdx_fail(ctx, TDX_ERR_ARG, std::string(who) + ": watershed id " + std::to_string(lohi[1]) + " above the largest supported one, " + std::to_string(TDX_CONNECTDOWN_MAX_ID));
    if (!any) return TDX_OK;        // a strip without ids: nothing to add
    const size_t m = size_t(lohi[1]) + 1;
    const unsigned dblocks = tdx_blocks_for(m, DEC_BLOCK_IDS);
    unsigned long long* table = static_cast<unsigned long long*>(ctx->scratch(TDX_S_A, m * 8));
    uint32_t* block_off = static_cast<uint32_t*>(ctx->scratch(TDX_S_I, size_t(dblocks) * 4 + 16));
    if (!table || !block_off) return tdx_fail(ctx, TDX_ERR_NOMEM, std::string(who) + ": out of device memory");
    unsigned long long* d_total = reinterpret_cast<unsigned long long*>(ctx->d_mail + TDX_MAIL_STAGE + 2);
    ev.begin(TDX_CONNECTDOWN_ARGMAX);
    TDX_HIP_CHECK(ctx, hipMemsetAsync(table, 0, m * 8, s));
    hipLaunchKernelGGL(argmax_kernel<false>, dim3(nblocks), dim3(256), 0, s, W, A, first, count, vec, w_nodata, table, static_cast<uint32_t*>(nullptr), mm + 2);
    ev.end(TDX_CONNECTDOWN_ARGMAX);
    ev.begin(TDX_CONNECTDOWN_DECODE);
    hipLaunchKernelGGL(present_count_kernel, dim3(dblocks), dim3(256), 0, s, table, m, block_off);
    hipLaunchKernelGGL(present_offsets_kernel, dim3(1), dim3(256), 0, s, block_off, dblocks, d_total);
    ev.end(TDX_CONNECTDOWN_DECODE);
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(ctx->h_mail + TDX_MAIL_STAGE, ctx->d_mail + TDX_MAIL_STAGE, 24, hipMemcpyDeviceToHost, s));
    TDX_HIP_CHECK(ctx, hipStreamSynchronize(s));
    uint32_t flag;
    memcpy(&flag, reinterpret_cast<const char*>(ctx->h_mail + TDX_MAIL_STAGE) + 8, 4);
    const size_t np = size_t(ctx->h_mail[TDX_MAIL_STAGE + 2]);
    uint32_t* first_cell = nullptr;
    if (flag) {   // a NaN somewhere: the first cell of every id decides whether it stands
        first_cell = static_cast<uint32_t*>(ctx->scratch(TDX_S_B, m * 4));
        if (!first_cell) return tdx_fail(ctx, TDX_ERR_NOMEM, std::string(who) + ": out of device memory");
        TDX_HIP_CHECK(ctx, hipMemsetAsync(first_cell, 0xff, m * 4, s));
        hipLaunchKernelGGL(argmax_kernel<true>, dim3(nblocks), dim3(256), 0, s, W, A, first, count, vec, w_nodata, static_cast<unsigned long long*>(nullptr), first_cell,
                           static_cast<uint32_t*>(nullptr));
    }
    uint8_t* out = static_cast<uint8_t*>(ctx->scratch(TDX_S_C, np * 20 + 16));
    if (!out) return tdx_fail(ctx, TDX_ERR_NOMEM, std::string(who) + ": out of device memory");
    int32_t* o_id = reinterpret_cast<int32_t*>(out);
    uint32_t* o_cell = reinterpret_cast<uint32_t*>(out + np * 4);
    float* o_val = reinterpret_cast<float*>(out + np * 8);
    uint32_t* o_first = reinterpret_cast<uint32_t*>(out + np * 12);
    float* o_fval = reinterpret_cast<float*>(out + np * 16);
    hipLaunchKernelGGL(decode_kernel, dim3(dblocks), dim3(256), 0, s, table, m, block_off, first_cell, A, o_id, o_cell, o_val, o_first, o_fval);
    res->ids.resize(np); cells.resize(np); res->ad8max.resize(np); firsts.resize(np); res->first_val.resize(np);
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(res->ids.data(), o_id, np * 4, hipMemcpyDeviceToHost, s));
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(cells.data(), o_cell, np * 4, hipMemcpyDeviceToHost, s));
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(res->ad8max.data(), o_val, np * 4, hipMemcpyDeviceToHost, s));
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(firsts.data(), o_first, np * 4, hipMemcpyDeviceToHost, s));
    TDX_HIP_CHECK(ctx, hipMemcpyAsync(res->first_val.data(), o_fval, np * 4, hipMemcpyDeviceToHost, s));
    TDX_HIP_CHECK(ctx, hipStreamSynchronize(s));
    return TDX_OK;
}

// whole: the points of a raster - an id whose first cell holds a NaN keeps that cell (the reference's strict >); a strip's part keeps both
void cells_to_points(const std::vector<uint32_t>& cells, const std::vector<uint32_t>& firsts, int nx, int64_t row_shift, bool whole, tdx_connectdown_points* res) {
    const size_t np = cells.size();
    res->x.resize(np); res->y.resize(np); res->first_x.assign(np, 0); res->first_y.assign(np, 0); res->first_is_nan.assign(np, 0);
    for (size_t i = 0; i < np; i++) {
        uint32_t c = cells[i];
        if (firsts[i] != NO_CELL) {
            if (whole) { c = firsts[i]; res->ad8max[i] = res->first_val[i]; }
            res->first_is_nan[i] = 1;
            res->first_x[i] = int32_t(firsts[i] % uint32_t(nx)); res->first_y[i] = int32_t(int64_t(firsts[i] / uint32_t(nx)) + row_shift);
        }
        res->x[i] = int32_t(c % uint32_t(nx)); res->y[i] = int32_t(int64_t(c / uint32_t(nx)) + row_shift);
    }
    res->mx = res->x; res->my = res->y;
    res->id_down.assign(np, 0);
}

int connectdown_impl(tdx_context* ctx, const int16_t* d_p, const int32_t* d_w, const float* d_ad8, int nx, int ny, int16_t p_nodata, int32_t w_nodata, int movedist,
                     tdx_connectdown_points* res, tdx_stats* stats) {
    TDX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    ctx->begin_call(stats);
    strip_mark(ctx, strip_single(nx, ny), "connectdown");
    PhaseEvents ev(ctx);
    std::vector<uint32_t> cells, firsts;
    {
        TdxSpan sp(ctx, TDX_K_MISC);
        if (int rc = argmax_run(ctx, nullptr, d_w, d_ad8, 0, size_t(nx) * size_t(ny), w_nodata, res, cells, firsts, ev, "tdx_connectdown")) return rc;
        if (stats) stats->launches[TDX_K_MISC] += 5;
    }
    cells_to_points(cells, firsts, nx, 0, true, res);
    const int64_t np = int64_t(cells.size());
    std::vector<int32_t> dist(size_t(np), 0), done(size_t(np), 0);
    {
        TdxSpan sp(ctx, TDX_K_ACCUM);
        ev.begin(TDX_CONNECTDOWN_WALK);
        const int rc = walk_run(ctx, WALK_CONNECTDOWN, d_p, d_w, nx, ny, 0, 0, ny, p_nodata, w_nodata, movedist, res->mx.data(), res->my.data(), dist.data(), done.data(),
                                res->id_down.data(), np, nullptr);
        if (rc != TDX_OK) return rc;
        ev.end(TDX_CONNECTDOWN_WALK);
        if (stats) stats->launches[TDX_K_ACCUM] += np ? 1 : 0;
    }
    ctx->end_call();
    ev.read(res->phase_ms);
    return TDX_OK;
}

bool walk_args_bad(const void* p, const void* side, int64_t nx, int64_t ny, int64_t n, const void* a, const void* b, const void* c) {
    return !p || !side || nx <= 0 || ny <= 0 || n < 0 || (n > 0 && (!a || !b || !c));
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------- MoveOutletsToStrm
extern "C" int tdx_moveoutlets_dev(tdx_context* ctx, const int16_t* d_p, const int32_t* d_src, int64_t nx, int64_t ny, int16_t p_nodata, int32_t src_nodata,
                                   int32_t maxdist, const int32_t* outlet_x, const int32_t* outlet_y, int64_t n_outlets, int32_t* out_x, int32_t* out_y,
                                   int32_t* dist_moved, tdx_stats* stats) {
    if (!ctx || walk_args_bad(d_p, d_src, nx, ny, n_outlets, out_x, out_y, dist_moved) || (n_outlets > 0 && (!outlet_x || !outlet_y)) || n_outlets > 0x3fffffff)
        return tdx_fail(ctx, TDX_ERR_ARG, "tdx_moveoutlets_dev: bad argument");
    if (too_big(nx, ny)) return tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip");
    TDX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    ctx->begin_call(stats);
    strip_mark(ctx, strip_single(int(nx), int(ny)), "moveoutlets");
    const size_t n = size_t(n_outlets);
    if (n) { memcpy(out_x, outlet_x, n * 4); memcpy(out_y, outlet_y, n * 4); }
    std::vector<int32_t> done(n, 0);
    for (size_t i = 0; i < n; i++) dist_moved[i] = 0;
    {
        TdxSpan sp(ctx, TDX_K_ACCUM);
        const int rc = walk_run(ctx, WALK_MOVEOUTLETS, d_p, d_src, int(nx), int(ny), 0, 0, int(ny), p_nodata, src_nodata, maxdist, out_x, out_y, dist_moved, done.data(),
                                nullptr, n_outlets, nullptr);
        if (rc != TDX_OK) return rc;
        if (stats) stats->launches[TDX_K_ACCUM] += n ? 1 : 0;
    }
    ctx->end_call();
    return TDX_OK;
}

extern "C" int tdx_moveoutlets(tdx_context* ctx, const int16_t* p, const int32_t* src, int64_t nx, int64_t ny, int16_t p_nodata, int32_t src_nodata, int32_t maxdist,
                               const int32_t* outlet_x, const int32_t* outlet_y, int64_t n_outlets, int32_t* out_x, int32_t* out_y, int32_t* dist_moved,
                               tdx_stats* stats) {
    if (!ctx || walk_args_bad(p, src, nx, ny, n_outlets, out_x, out_y, dist_moved) || (n_outlets > 0 && (!outlet_x || !outlet_y)))
        return tdx_fail(ctx, TDX_ERR_ARG, "tdx_moveoutlets: bad argument");
    if (too_big(nx, ny)) return tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip");
    HostCall h(ctx, nx, ny);
    int16_t* d_p = h.in(TDX_S_IO0, p);
    int32_t* d_s = h.in(TDX_S_IO1, src);
    if (h.error) return h.error;
    return h.finish(tdx_moveoutlets_dev(ctx, d_p, d_s, nx, ny, p_nodata, src_nodata, maxdist, outlet_x, outlet_y, n_outlets, out_x, out_y, dist_moved, stats));
}

extern "C" int tdx_moveoutlets_strip(tdx_context* ctx, const tdx_comm* comm, const int16_t* d_p, const int32_t* d_src, int64_t nx, int64_t ny_local, int64_t row0,
                                     int64_t ny_total, int16_t p_nodata, int32_t src_nodata, int32_t maxdist, int32_t* state_x, int32_t* state_y, int32_t* state_dist,
                                     int32_t* state_done, int64_t n_outlets, int64_t* n_moved, tdx_stats* stats) {
    if (!ctx || walk_args_bad(d_p, d_src, nx, ny_local, n_outlets, state_x, state_y, state_dist) || (n_outlets > 0 && !state_done) || row0 < 0 ||
        row0 + ny_local > ny_total || ny_total > 0x7ffffff0 || n_outlets > 0x3fffffff)
        return tdx_fail(ctx, TDX_ERR_ARG, "tdx_moveoutlets_strip: bad argument");
    if (too_big(nx, ny_local + 2)) return tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip");
    TDX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    ctx->begin_call(stats);
    strip_mark(ctx, strip_from_comm(comm, int(nx), int(ny_local)), "moveoutlets");
    {
        TdxSpan sp(ctx, TDX_K_ACCUM);
        const int rc = walk_run(ctx, WALK_MOVEOUTLETS, d_p, d_src, int(nx), int(ny_total), int(row0) - 1, int(row0), int(row0 + ny_local), p_nodata, src_nodata, maxdist,
                                state_x, state_y, state_dist, state_done, nullptr, n_outlets, n_moved);
        if (rc != TDX_OK) return rc;
        if (stats) stats->launches[TDX_K_ACCUM] += n_outlets ? 1 : 0;
    }
    ctx->end_call();
    return TDX_OK;
}

// ---------------------------------------------------------------------------------------------------------------- ConnectDown
extern "C" int tdx_connectdown_dev(tdx_context* ctx, const int16_t* d_p, const int32_t* d_w, const float* d_ad8, int64_t nx, int64_t ny, int16_t p_nodata,
                                   int32_t w_nodata, int32_t movedist, tdx_connectdown_points** points, tdx_stats* stats) {
    if (!ctx || !d_p || !d_w || !d_ad8 || !points || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_connectdown_dev: bad argument");
    if (too_big(nx, ny)) return tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip");
    *points = nullptr;
    tdx_connectdown_points* res = new tdx_connectdown_points;
    const int rc = connectdown_impl(ctx, d_p, d_w, d_ad8, int(nx), int(ny), p_nodata, w_nodata, movedist, res, stats);
    if (rc != TDX_OK) { delete res; return rc; }
    *points = res;
    return TDX_OK;
}

extern "C" int tdx_connectdown(tdx_context* ctx, const int16_t* p, const int32_t* w, const float* ad8, int64_t nx, int64_t ny, int16_t p_nodata, int32_t w_nodata,
                               int32_t movedist, tdx_connectdown_points** points, tdx_stats* stats) {
    if (!ctx || !p || !w || !ad8 || !points || nx <= 0 || ny <= 0) return tdx_fail(ctx, TDX_ERR_ARG, "tdx_connectdown: bad argument");
    if (too_big(nx, ny)) return tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip");
    HostCall h(ctx, nx, ny);
    int16_t* d_p = h.in(TDX_S_IO0, p);
    int32_t* d_w = h.in(TDX_S_IO1, w);
    float* d_a = h.in(TDX_S_IO2, ad8);
    if (h.error) return h.error;
    return h.finish(tdx_connectdown_dev(ctx, d_p, d_w, d_a, nx, ny, p_nodata, w_nodata, movedist, points, stats));
}

extern "C" int64_t tdx_connectdown_points_count(const tdx_connectdown_points* points) { return points ? int64_t(points->ids.size()) : 0; }
extern "C" void tdx_connectdown_points_copy(const tdx_connectdown_points* pt, int32_t* ids, int32_t* x, int32_t* y, float* ad8max, int32_t* moved_x, int32_t* moved_y,
                                            int32_t* id_down, double* phase_ms) {
    if (!pt) return;
    const size_t nb = pt->ids.size() * 4;
    if (nb) {
        if (ids) memcpy(ids, pt->ids.data(), nb);
        if (x) memcpy(x, pt->x.data(), nb);
        if (y) memcpy(y, pt->y.data(), nb);
        if (ad8max) memcpy(ad8max, pt->ad8max.data(), nb);
        if (moved_x) memcpy(moved_x, pt->mx.data(), nb);
        if (moved_y) memcpy(moved_y, pt->my.data(), nb);
        if (id_down) memcpy(id_down, pt->id_down.data(), nb);
    }
    if (phase_ms) memcpy(phase_ms, pt->phase_ms, sizeof pt->phase_ms);
}
extern "C" void tdx_connectdown_points_free(tdx_connectdown_points* points) { delete points; }
extern "C" int tdx_connectdown_points_set_moved(tdx_connectdown_points* pt, const int32_t* moved_x, const int32_t* moved_y, const int32_t* id_down) {
    if (!pt || (!pt->ids.empty() && (!moved_x || !moved_y || !id_down))) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_connectdown_points_set_moved: bad argument");
    const size_t n = pt->ids.size();
    pt->mx.assign(moved_x, moved_x + n); pt->my.assign(moved_y, moved_y + n); pt->id_down.assign(id_down, id_down + n);
    return TDX_OK;
}

extern "C" int tdx_connectdown_strip(tdx_context* ctx, const tdx_comm* comm, const int32_t* d_w, const float* d_ad8, int64_t nx, int64_t ny_local, int64_t row0,
                                     int32_t w_nodata, tdx_connectdown_points** part, tdx_stats* stats) {
    if (!ctx || !d_w || !d_ad8 || !part || nx <= 0 || ny_local <= 0 || row0 < 0 || row0 + ny_local > 0x7ffffff0)
        return tdx_fail(ctx, TDX_ERR_ARG, "tdx_connectdown_strip: bad argument");
    if (too_big(nx, ny_local + 2)) return tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip");
    *part = nullptr;
    TDX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const Strip st = strip_from_comm(comm, int(nx), int(ny_local));
    tdx_connectdown_points* res = new tdx_connectdown_points;
    ctx->begin_call(stats);
    strip_mark(ctx, st, "connectdown");
    PhaseEvents ev(ctx);
    std::vector<uint32_t> cells, firsts;
    int rc;
    {
        TdxSpan sp(ctx, TDX_K_MISC);
        rc = argmax_run(ctx, &st, d_w, d_ad8, size_t(nx), size_t(nx) * size_t(ny_local), w_nodata, res, cells, firsts, ev, "tdx_connectdown_strip");   // the owned rows: 1 .. ny_local
    }
    if (rc != TDX_OK) { delete res; return rc; }
    cells_to_points(cells, firsts, int(nx), row0 - 1, false, res);
    ctx->end_call();
    ev.read(res->phase_ms);
    *part = res;
    return TDX_OK;
}

extern "C" int tdx_connectdown_merge(const tdx_connectdown_points* const* parts, int64_t n_parts, tdx_connectdown_points** points) {
    if (!parts || n_parts <= 0 || !points) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_connectdown_merge: bad argument");
    for (int64_t k = 0; k < n_parts; k++)
        if (!parts[k]) return tdx_fail(nullptr, TDX_ERR_ARG, "tdx_connectdown_merge: bad argument");
    tdx_connectdown_points* res = new tdx_connectdown_points;
    // a k-way merge by id over lists that are sorted by id.  One rank starts from the id's first cell and replaces it with a strict > (src/ConnectDown.cpp:
    // 223-244): a NaN there is never replaced, a NaN anywhere else never chosen.  So the first strip that holds the id decides whether its first cell
    // stands; otherwise the strips' maxima over the cells that are not NaN meet in strip order with that strict >, which is row-major-first.
    std::vector<size_t> at(size_t(n_parts), 0);
    for (;;) {
        int64_t best = -1;
        for (int64_t k = 0; k < n_parts; k++)
            if (at[size_t(k)] < parts[k]->ids.size() && (best < 0 || parts[k]->ids[at[size_t(k)]] < parts[best]->ids[at[size_t(best)]])) best = k;
        if (best < 0) break;
        const int32_t id = parts[best]->ids[at[size_t(best)]];
        int32_t x = 0, y = 0; float v = 0.f; bool have = false, locked = false;
        for (int64_t k = 0; k < n_parts; k++) {
            const tdx_connectdown_points* pk = parts[k];
            size_t& i = at[size_t(k)];
            if (i < pk->ids.size() && pk->ids[i] == id) {
                if (!have && i < pk->first_is_nan.size() && pk->first_is_nan[i]) { x = pk->first_x[i]; y = pk->first_y[i]; v = pk->first_val[i]; locked = true; }
                else if (!locked && (!have || pk->ad8max[i] > v)) { x = pk->x[i]; y = pk->y[i]; v = pk->ad8max[i]; }
                have = true;
                i++;
            }
        }
        res->ids.push_back(id); res->x.push_back(x); res->y.push_back(y); res->ad8max.push_back(v);
    }
    for (int64_t k = 0; k < n_parts; k++)
        for (int j = 0; j < TDX_CONNECTDOWN_WALK; j++) res->phase_ms[j] = std::max(res->phase_ms[j], parts[k]->phase_ms[j]);
    res->mx = res->x; res->my = res->y; res->id_down.assign(res->ids.size(), 0);
    *points = res;
    return TDX_OK;
}

extern "C" int tdx_connectdown_walk_strip(tdx_context* ctx, const tdx_comm* comm, const int16_t* d_p, const int32_t* d_w, int64_t nx, int64_t ny_local, int64_t row0,
                                          int64_t ny_total, int32_t movedist, int32_t* state_x, int32_t* state_y, int32_t* state_dist, int32_t* state_done,
                                          int32_t* id_down, int64_t n_points, int64_t* n_moved, tdx_stats* stats) {
    if (!ctx || walk_args_bad(d_p, d_w, nx, ny_local, n_points, state_x, state_y, state_dist) || (n_points > 0 && (!state_done || !id_down)) || row0 < 0 ||
        row0 + ny_local > ny_total || ny_total > 0x7ffffff0 || n_points > 0x3fffffff)
        return tdx_fail(ctx, TDX_ERR_ARG, "tdx_connectdown_walk_strip: bad argument");
    if (too_big(nx, ny_local + 2)) return tdx_fail(ctx, TDX_ERR_ARG, "raster larger than 2^32 cells per device strip");
    TDX_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    ctx->begin_call(stats);
    strip_mark(ctx, strip_from_comm(comm, int(nx), int(ny_local)), "connectdown");
    {
        TdxSpan sp(ctx, TDX_K_ACCUM);
        const int rc = walk_run(ctx, WALK_CONNECTDOWN, d_p, d_w, int(nx), int(ny_total), int(row0) - 1, int(row0), int(row0 + ny_local), 0, 0, movedist, state_x, state_y,
                                state_dist, state_done, id_down, n_points, n_moved);
        if (rc != TDX_OK) return rc;
        if (stats) stats->launches[TDX_K_ACCUM] += n_points ? 1 : 0;
    }
    ctx->end_call();
    return TDX_OK;
}
