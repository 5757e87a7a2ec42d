// The host schedule of a tile dependency sweep (d8_sweep.hpp: the D8 family; dinf_sweep.hpp / areadinf.hip: AreaDinf and DinfDecayAccum), written once.
// A sweep runs over TWO tile geometries of the same arrays (its state is the work array alone): small tiles carry the BULK rounds, in which every tile of
// the raster is active and what counts is how many tiles a CU works on at once; 64 x 64 tiles carry the TAIL, where a round is one tile crossing of the
// longest dependency chain and fewer crossings win.  Between the two the activation flags are handed over (flags_down_kernel / flags_up_kernel); with
// neighbouring strips the halo rows are exchanged until no strip sees a change.  What the two families do differently is a named field of Params; the tile
// kernels and the record type of the exchange stay with the callers (`launch`, `exchange`).
#pragma once
#include "strips.hpp"
#include "tile_relax.hpp"

namespace sweepsched {

// activation flags between the two tile geometries (a 64 x 64 tile = 2 x 2 tiles of 32 x 32, sh = 1, or 4 x 4 tiles of 16 x 16, sh = 2)
static __global__ __launch_bounds__(256) void flags_down_kernel(const uint32_t* __restrict__ f64, int tiles_x64, uint32_t* __restrict__ f32, int tiles_x32,
                                                                int tiles_y32, int sh) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= tiles_x32 * tiles_y32) return;
    const int tx = t % tiles_x32, ty = t / tiles_x32;
    f32[t] = f64[(ty >> sh) * tiles_x64 + (tx >> sh)] ? tilek::FLAG_FULL : 0u;
}
static __global__ __launch_bounds__(256) void flags_up_kernel(uint32_t* __restrict__ f32, int tiles_x32, int tiles_y32, uint32_t* __restrict__ f64, int tiles_x64, int sh) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= tiles_x32 * tiles_y32) return;
    if (f32[t]) {
        f32[t] = 0u;
        const int tx = t % tiles_x32, ty = t / tiles_x32;
        f64[(ty >> sh) * tiles_x64 + (tx >> sh)] = tilek::FLAG_HALO;   // walks only: the bulk sweeps have run
    }
}

struct Params {
    int bulk_ts;                     // edge of the bulk rounds' tiles.  D8: 32.  D-infinity: 32, or 16 (one wave per tile) for AreaDinf's large rasters
    int bulk_grid_per_cu;            // workgroups per CU of a full bulk round.  16 for 32 x 32 tiles; 48 for 16 x 16 tiles (13.6 KB of LDS, one wave: more fit a CU)
    unsigned long long bulk_until;   // the bulk phase ends when a round has at most this many active small tiles (0: no bulk phase).  A policy constant of each family
    int max_sweeps_bulk;             // TileGeom::max_sweeps (lockstep sweeps of a fresh tile) of the two geometries.  D8 gives both the same number (TDX_D8_BULK_SWEEPS);
    int max_sweeps_tail;             // D-infinity's TDX_DINF_BULK_SWEEPS has only ever reached the bulk tiles, its tail keeps the constant
    bool exchange_after_bulk;        // several strips: exchange straight after a bulk phase, before the first tail round.  D-infinity yes (measured the same step time, and
                                     // its segment trace shows the two phases apart); D8 no: its tail starts at once
    const char* phase_bulk;          // ctx->phase during the two phases (segment trace).  D-infinity names them; D8 passes nullptr and keeps what the calling tool set
    const char* phase_tail;
    const char* rounds_label;        // TDX_DEBUG_ROUNDS: the line in front of a schedule's active tiles per round, a format of (tiles, tile edge); scripts read it
};

// called with begin = true before a schedule's first round and with begin = false after every collected batch (D-infinity: the phase clocks of TDX_DEBUG_ROUNDS=1)
using BatchHook = std::function<int(bool small, const RoundSchedule& run, bool begin)>;

// Runs the sweep to the global fixed point.  The work array must be initialised and its halo rows exchanged.
//   launch(small, geom, grid, stream, list, count, flags_cur, flags_next, list_next, pull_max)   one round of the small / the 64 x 64 tile kernel
//   exchange(flags, tiles_x, &changed, left)   the strips' halo rows of the work array (strip_exchange with the global vote), raising the 64 x 64 tiles' flags
// counts: COUNT_RING * 2 words of the caller's; the flags and lists of the two geometries live in the scratch slots TDX_S_L and TDX_S_G.
template <class Launch, class Exchange>
static int run(tdx_context* ctx, const Strip& st, const Params& P, unsigned long long* counts, Launch&& launch, Exchange&& exchange, int64_t* rounds_out,
               int64_t* launches_out, int64_t* outer_out, const BatchHook& hook = nullptr) {
    hipStream_t s = ctx->stream;
    tilek::TileGeom geom = tilek::make_geom(st.nx, st.ny_arr, st.y0, st.y1);
    geom.max_sweeps = P.max_sweeps_tail;
    tilek::TileGeom geom32 = geom;
    geom32.tiles_x = (st.nx + P.bulk_ts - 1) / P.bulk_ts; geom32.tiles_y = (st.ny_arr + P.bulk_ts - 1) / P.bulk_ts;
    geom32.max_sweeps = P.max_sweeps_bulk;
    const int bulk_sh = P.bulk_ts == 16 ? 2 : 1;
    const size_t ntiles = size_t(geom.tiles_x) * size_t(geom.tiles_y), ntiles32 = size_t(geom32.tiles_x) * size_t(geom32.tiles_y);
    uint32_t* flags = static_cast<uint32_t*>(ctx->scratch(TDX_S_L, ntiles * 4 * (1 + tilek::SCHED_LIST_WORDS)));
    uint32_t* flags32 = static_cast<uint32_t*>(ctx->scratch(TDX_S_G, ntiles32 * 4 * (1 + tilek::SCHED_LIST_WORDS)));
    if (!flags || !flags32) return TDX_ERR_NOMEM;
    const tilek::Sched sched{flags, flags + ntiles, counts}, sched32{flags32, flags32 + ntiles32, counts};
    // runs one geometry until no tile is active, or (stop_at > 0) until a round has at most stop_at active tiles, or (max_rounds > 0) until that many rounds
    // have run - a multi-strip tail exchanges its boundary rows every few rounds instead of running every strip to its local fixed point first; says whether
    // tiles are still active (their flags of the next round are then in the schedule's flag half *parity_out)
    auto run_rounds = [&](bool small, const tilek::TileGeom& gg, const tilek::Sched& sc, unsigned long long stop_at, bool* active_left, int* parity_out,
                          int max_rounds = 0) -> int {
        RoundSchedule runner(ctx, s, gg, sc, ctx->h_mail + TDX_MAIL_RUN_A,
                             [&](const tilek::TileGeom& rg, unsigned grid, hipStream_t ls, const uint32_t* list, unsigned long long* count, uint32_t* fcur, uint32_t* fnext,
                                 uint32_t* lnext, unsigned pull_max) { launch(small, rg, grid, ls, list, count, fcur, fnext, lnext, pull_max); });
        if (max_rounds > 0) { runner.batch = max_rounds; runner.batch_max = max_rounds; }
        if (small) { runner.grid_full = unsigned(std::min(runner.ntiles, P.bulk_grid_per_cu * ctx->num_cus)); runner.grid_small = unsigned(std::min(runner.ntiles, 4 * ctx->num_cus)); }
        static const bool print_rounds = getenv("TDX_DEBUG_ROUNDS") != nullptr;   // active tiles per round on stderr
        runner.print_counts = print_rounds;
        if (print_rounds) fprintf(stderr, P.rounds_label, runner.ntiles, small ? P.bulk_ts : 64);
        int rcl = hook ? hook(small, runner, true) : TDX_OK;
        if (rcl != TDX_OK) return rcl;
        rcl = runner.start();
        if (rcl != TDX_OK) return rcl;
        *active_left = false;
        while (!runner.done) {
            rcl = runner.enqueue();
            if (rcl != TDX_OK) return rcl;
            TDX_HIP_CHECK(ctx, hipStreamSynchronize(s));
            runner.collect();
            if (hook) { rcl = hook(small, runner, false); if (rcl != TDX_OK) return rcl; }
            if (!runner.done && stop_at > 0 && runner.last_count <= stop_at) { *active_left = true; *parity_out = runner.parity; break; }
            if (!runner.done && max_rounds > 0 && runner.rounds >= max_rounds) { *active_left = true; *parity_out = runner.parity; break; }
        }
        if (rounds_out) *rounds_out += runner.rounds;
        if (launches_out) *launches_out += runner.launches;
        return TDX_OK;
    };
    hipLaunchKernelGGL(tilek::fill_u32_kernel, dim3(tdx_blocks_for(ntiles, 256)), dim3(256), 0, s, flags, tilek::FLAG_FULL, ntiles);   // round 0: every tile
    bool bulk = P.bulk_until > 0 && ntiles32 > P.bulk_until;
    int rc;
    for (;;) {
        bool left = false, bulk_just_ran = false;
        int par = 0;
        if (bulk) {
            if (P.phase_bulk) ctx->phase = P.phase_bulk;
            // bulk phase on the small tiles: every small tile under an active 64-tile starts active
            hipLaunchKernelGGL(flags_down_kernel, dim3(tdx_blocks_for(ntiles32, 256)), dim3(256), 0, s, flags, geom.tiles_x, flags32, geom32.tiles_x, geom32.tiles_y, bulk_sh);
            TDX_HIP_CHECK(ctx, hipMemsetAsync(flags, 0, ntiles * 4, s));
            rc = run_rounds(true, geom32, sched32, P.bulk_until, &left, &par);
            if (rc != TDX_OK) return rc;
            if (left) {   // what is still active goes on in 64 x 64 tiles
                uint32_t* f32next = par ? sched32.list + 2 * ntiles32 : sched32.flags;
                hipLaunchKernelGGL(flags_up_kernel, dim3(tdx_blocks_for(ntiles32, 256)), dim3(256), 0, s, f32next, geom32.tiles_x, geom32.tiles_y, flags, geom.tiles_x, bulk_sh);
            }
            bulk = false;   // (strip re-activations are few tiles: 64 x 64)
            bulk_just_ran = true;
        } else left = true;
        // (exchange_after_bulk: with neighbours the bulk phase is followed by an exchange at once: the tail's first rounds then see what the neighbours' bulk phases
        // finished - the step time is the same either way: 311.4 against 311.2 ms projected at BASELINE.json configs[4])
        if (left && !(P.exchange_after_bulk && bulk_just_ran && st.multi())) {
            if (P.phase_tail) ctx->phase = P.phase_tail;
            // Multi-strip tail: at most `eager` rounds between two exchanges.  A strip that runs to its local fixed point first makes every flow path
            // that crosses a strip boundary wait for the longest chain ANYWHERE in the strip it enters - at BASELINE.json configs[4] 47 crossings x
            // ~10 ms (profiles/r05b_projection_decay.txt); with frequent exchanges the paths advance side by side, as on one GPU.
            const int eager_env = getenv("TDX_SWEEP_EAGER_ROUNDS") ? std::max(0, atoi(getenv("TDX_SWEEP_EAGER_ROUNDS"))) : 8;   // (0: local fixed points)
            rc = run_rounds(false, geom, sched, 0, &left, &par, st.multi() ? eager_env : 0);
            if (rc != TDX_OK) return rc;
            if (left && par)   // stopped with tiles still active: the next schedule starts from the first flag half
                hipLaunchKernelGGL(tilek::flags_fold_kernel, dim3(tdx_blocks_for(ntiles, 256)), dim3(256), 0, s, sched.flags, sched.list + 2 * ntiles, int(ntiles));
        }
        if (!st.multi()) break;
        // the neighbours' boundary rows: cells finished there release the owned cells they drain into (the reference's addBorders() + queue refill); tiles that
        // see a changed halo cell run again
        int64_t changed = 0;
        rc = exchange(flags, geom.tiles_x, &changed, left ? 1 : 0);
        if (rc != TDX_OK) return rc;
        if (changed == 0) break;
        if (outer_out) (*outer_out)++;
    }
    return TDX_OK;
}

}  // namespace sweepsched
