// The tile routine of the D-infinity dependency sweep (AreaDinf, DinfDecayAccum), a template over the tile edge TSZ = 64 | 32 | 16.
// 32 x 32 tiles (28 KB of LDS: five tiles per CU) carry the BULK rounds, in which every tile of the raster is active and a
// tile's time is its longest in-tile chain - what counts is how many tiles a CU works on at once; 64 x 64 tiles (113 KB, one per
// CU) carry the TAIL, where a round is one tile crossing of the longest dependency chain and fewer crossings win.
// 16 x 16 tiles, ONE wave per tile (no workgroup barrier in the hop loop, 13 KB of LDS) - the variant VERDICT r04 asked to be
// measured for the bulk rounds (TDX_DINF_BULK_TILE=16; docs/experiments_r05.md has what it did).
// Part of areadinf.hip: included there once, after the helpers of its namespace that the routine uses (Nbr8, load_nbrs, pending, pending_bits,
// QCAP, wall_clock64); the evaluation policies (AreaEval, DecayEval) are template arguments.
#pragma once
namespace dsweep {
template <int TSZ>
struct Dim {
    static constexpr int TS = TSZ, LH = TSZ + 2;
    static constexpr int NT = TSZ == 64 ? 1024 : (TSZ == 32 ? 256 : 64);   // threads per tile: lane (tid % TS, tid / TS) owns column lx and RPL consecutive rows
    static constexpr int RPL = TS * TS / NT;   // cells per lane
    static constexpr int NSTAGE = (LH * LH + NT - 1) / NT;
    static constexpr int QLEN = TS == 16 ? 64 : (TS == 32 ? 128 : QCAP);   // hand-over queue (a fork whose two branches become ready at once; an overflow re-runs the tile)
    template <bool HAS_DM>
    static constexpr bool USE_CW = TS <= 32 || !HAS_DM;
};
constexpr int BULK_SWEEPS = 6;    // lockstep sweeps of a fresh tile (measured, AreaDinf at 32768^2 / 16384^2: 1: 220.8 / 78.2 ms, 3: 219.2 / 77.5, 6: 217.6 / 77.3, 8: 219.2 / 76.2, 12: 221.7 / 77.6, 16: 221.7 / 78.1; profiles/r06ah_*)

template <int TSZ, bool HAS_W, bool HAS_DM>
struct Lds {
    static constexpr int TS = Dim<TSZ>::TS, LH = Dim<TSZ>::LH, QLEN = Dim<TSZ>::QLEN;
    double2 p[LH * LH];            // outflow proportions of tile + ring
    float out[LH * LH];
    float dm[HAS_DM ? LH * LH : 1];
    float w[HAS_W ? TS * TS : 1];
    uint32_t info[TS * TS];
    uint32_t cnt[TS * TS / 4];     // one byte per cell: contributors still pending (255: not a pending cell of this rank)
    uint32_t tw[TS * TS];          // the cell's targets inside the tile, made once per activation: index t0 [0:12) t1 [12:24), "is in the tile" bits 24 / 25,
                                   // "exists, outside the tile" bits 26 / 27 (the walks read them with the info word: no direction arithmetic per hop)
    uint32_t spare[64];            // what a target that does not exist decrements (one word per lane: the walk has no branch around its two atomics)
    uint32_t cw[Dim<TSZ>::template USE_CW<HAS_DM> ? TS * TS : 1];   // the cell's first three contributors, made once per activation: per slot i, bits [9i, 9i + 8) the contributor's
                                   // element offset from the cell (signed), bit 9i + 8 which of its two proportions; bit 27 = info bit 8 (a neighbour is
                                   // missing), bits [28:32) the number of contributors.  (Not where it would not fit: the 64 x 64 decay tile.)
    double dx[TS];                 // cell size of the tile's rows (the unweighted increment)
    uint16_t q[2][QLEN];           // ready cells handed on to the next phase
    unsigned nq[2];
    int rim;                       // RES_* rim bits: neighbouring tiles that receive flow from cells finished in this activation
    int over;                      // the queue overflowed: the tile runs again (ready cells are re-discovered from the values)
    int wrote;                     // some lane wrote a result back in this activation
    unsigned long long dbg[10];    // TDX_DEBUG_ROUNDS=1: this workgroup's phase clocks of the launch; [8] cells pending when staged, [9] cells evaluated
};

// targets of a finished cell that lie outside the tile: those tiles have to look again
template <int TSZ>
__device__ __forceinline__ int rim_bits(unsigned inf, int cx, int ly) {
    constexpr int TS = Dim<TSZ>::TS;
    int bits = 0;
    const int s1 = int((inf >> 9) & 7u) + 1;
#pragma unroll
    for (int t = 0; t < 2; t++) {
        if (!((inf >> (12 + t)) & 1u)) continue;
        const int k = t == 0 ? s1 : (s1 % 8 + 1);
        const int nx2 = cx + d1(k), ny2 = ly + d2(k);
        if (nx2 < 0 || nx2 >= TS || ny2 < 0 || ny2 >= TS)
            bits |= ny2 < 0 ? (nx2 < 0 ? 16 : (nx2 >= TS ? 32 : 1)) : (ny2 >= TS ? (nx2 < 0 ? 64 : (nx2 >= TS ? 128 : 2)) : (nx2 < 0 ? 4 : 8));
    }
    return bits;
}

// Evaluation of a cell from the contributors that EXIST, in k order (most cells have one to three).  Reading all eight neighbour records and stepping
// through eight predicated blocks (Eval::eval on a Nbr8) was most of a walker's ~370 instructions per hop and of a lockstep sweep's work per cell.
// The first three contributors' values and proportions are requested together (one LDS latency; an empty slot reads the cell itself and is not
// folded), further ones - confluences - in a loop.  CHECK: the lockstep sweeps do not know whether the cell is ready - a contributor that is still
// pending makes the function return false before anything is folded; the walkers only reach cells whose last contributor has just finished.
// Same operations in the same order as Eval::eval (which the verifier of areadinf.hip keeps using: an independent second form).
// TDX_DSWEEP_DENSE restores the old form everywhere (A/B).
template <bool CHECK, class Eval, int TSZ, bool HAS_W, bool HAS_DM>
__device__ __forceinline__ bool eval_cell(const Eval& ev, const Lds<TSZ, HAS_W, HAS_DM>& S, int c, int cl, int ly, unsigned inf, int contcheck, float* result) {
    constexpr int LH = Dim<TSZ>::LH;
    const float wv = HAS_W ? S.w[c] : 0.f;
    const double dxv = S.dx[ly];
#ifdef TDX_DSWEEP_DENSE
    Nbr8 nb;
    load_nbrs<Lds<TSZ, HAS_W, HAS_DM>, HAS_DM, LH>(S, cl, nb);
    if (CHECK && (inf & 0xFFu & pending_bits(nb)) != 0u) return false;
    *result = ev.eval(nb, wv, dxv, inf, contcheck, HAS_W);
    return true;
#else
    unsigned m = inf & 0xFFu;
    int kk[3];
    float vv[3], dd[3];
    double pp[3];
    if constexpr (Dim<TSZ>::template USE_CW<HAS_DM>) {
        const unsigned cw = S.cw[c];
        const int ncon = int(cw >> 28);
#pragma unroll
        for (int i = 0; i < 3; i++) {
            kk[i] = i < ncon ? 1 : 0;                           // (only "is there an i-th contributor" is looked at below)
            const int n = cl + __builtin_amdgcn_sbfe(int(cw), 9 * i, 8);
            vv[i] = S.out[n];
            pp[i] = reinterpret_cast<const double*>(&S.p[n])[(cw >> (9 * i + 8)) & 1u];
            dd[i] = HAS_DM ? S.dm[n] : 0.f;
        }
        if (ncon > 3) { m &= m - 1u; m &= m - 1u; m &= m - 1u; } else m = 0u;
    } else {
#pragma unroll
        for (int i = 0; i < 3; i++) {
            kk[i] = m ? __ffs(int(m)) : 0;                       // 1..8, 0 = no further contributor
            m &= m - 1u;                                         // (0 stays 0)
            const int n = kk[i] ? cl + d2(kk[i]) * LH + d1(kk[i]) : cl;
            vv[i] = S.out[n];
            pp[i] = reinterpret_cast<const double*>(&S.p[n])[(inf >> (15 + kk[i])) & 1u];   // bit 16 + k - 1: the contributor's second proportion
            dd[i] = HAS_DM ? S.dm[n] : 0.f;
        }
    }
    if (CHECK) {
        bool pend = false;
#pragma unroll
        for (int i = 0; i < 3; i++) pend = pend || (kk[i] != 0 && pending(vv[i]));
        for (unsigned mm = m; mm && !pend; mm &= mm - 1u) {
            const int k = __ffs(int(mm));
            pend = pending(S.out[cl + d2(k) * LH + d1(k)]);
        }
        if (pend) return false;
    }
    float acc = ev.begin(wv, dxv, HAS_W);
    bool con = (inf & 0x100u) != 0u;
#pragma unroll
    for (int i = 0; i < 3; i++)
        if (kk[i]) ev.fold(acc, con, vv[i], pp[i], dd[i]);
    while (m) {                                              // a fourth ... eighth contributor
        const int k = __ffs(int(m));
        m &= m - 1u;
        const int n = cl + d2(k) * LH + d1(k);
        ev.fold(acc, con, S.out[n], reinterpret_cast<const double*>(&S.p[n])[(inf >> (15 + k)) & 1u], HAS_DM ? S.dm[n] : 0.f);
    }
    *result = ev.end(acc, con, wv, dxv, HAS_W, contcheck);
    return true;
#endif
}

template <class Eval, int TSZ, bool HAS_W, bool HAS_DM>
__device__ __forceinline__ int sweep_tile(const Eval& ev, const tilek::TileGeom& g, int tile, bool full, Lds<TSZ, HAS_W, HAS_DM>& S, const double2* __restrict__ P,
                                          const float* __restrict__ W, const float* __restrict__ DM, const uint32_t* __restrict__ INFO,
                                          const RowProp* __restrict__ rows, float* __restrict__ OUT, float out_nodata, int contcheck,
                                          unsigned long long* __restrict__ dbg) {
    constexpr int TS = Dim<TSZ>::TS, LH = Dim<TSZ>::LH, NT = Dim<TSZ>::NT, RPL = Dim<TSZ>::RPL, NSTAGE = Dim<TSZ>::NSTAGE, QLEN = Dim<TSZ>::QLEN;
    const int tid = threadIdx.x, lx = tid % TS, ry0 = (tid / TS) * RPL;
    const int tx = tile % g.tiles_x, ty = tile / g.tiles_x;
    const int x0 = tx * TS, y0 = ty * TS;
    const unsigned long long tc0 = dbg ? wall_clock64() : 0ull;
    unsigned long long hops = 0, nphase = 0;
    if (tid == 0) { S.rim = 0; S.over = 0; S.nq[0] = 0u; S.nq[1] = 0u; S.wrote = 0; }
    // ---- stage: every load of a lane is issued before the first LDS store (ONE memory latency per activation); addresses
    // are clamped into the raster and validity is applied afterwards (a load inside a divergent branch is waited for at once)
    {
        float so[NSTAGE], sd[HAS_DM ? NSTAGE : 1];
        double2 sp[NSTAGE];
        uint32_t si[RPL];
        float sw[HAS_W ? RPL : 1];
        unsigned ok = 0;
#pragma unroll
        for (int i = 0; i < NSTAGE; i++) {
            const int e = tid + i * NT, ec = e < LH * LH ? e : LH * LH - 1;
            const int wy = ec / LH, wx = ec - wy * LH;
            const int gx = x0 - 1 + wx, gy = y0 - 1 + wy;
            if (gx >= 0 && gx < g.nx && gy >= 0 && gy < g.ny) ok |= 1u << i;
            const int gxc = gx < 0 ? 0 : (gx >= g.nx ? g.nx - 1 : gx), gyc = gy < 0 ? 0 : (gy >= g.ny ? g.ny - 1 : gy);
            const size_t idx = size_t(gyc) * size_t(g.nx) + size_t(gxc);
            so[i] = OUT[idx];
            sp[i] = P[idx];
            if (HAS_DM) sd[i] = DM[idx];
        }
        unsigned oki = 0;
#pragma unroll
        for (int r = 0; r < RPL; r++) {
            const int gx = x0 + lx, gy = y0 + ry0 + r;
            if (gx < g.nx && gy < g.ny) oki |= 1u << r;
            const size_t idx = size_t(gy >= g.ny ? g.ny - 1 : gy) * size_t(g.nx) + size_t(gx >= g.nx ? g.nx - 1 : gx);
            si[r] = INFO[idx];
            if (HAS_W) sw[r] = W[idx];
        }
        double dxrow = 0.;
        if (tid < TS) dxrow = rows[y0 + tid >= g.ny ? g.ny - 1 : y0 + tid].dx;
#pragma unroll
        for (int i = 0; i < NSTAGE; i++) {
            const int e = tid + i * NT;
            if (e < LH * LH) {
                const bool in = (ok >> i) & 1u;
                S.out[e] = in ? so[i] : out_nodata;
                S.p[e] = in ? sp[i] : make_double2(0., 0.);
                if (HAS_DM) S.dm[e] = in ? sd[i] : 0.f;
            }
        }
#pragma unroll
        for (int r = 0; r < RPL; r++) {
            const unsigned inf = ((oki >> r) & 1u) ? si[r] : 0u;
            S.info[(ry0 + r) * TS + lx] = inf;
            if (HAS_W) S.w[(ry0 + r) * TS + lx] = ((oki >> r) & 1u) ? sw[r] : 0.f;
            unsigned tw = 0u;
            const int s1 = int((inf >> 9) & 7u) + 1;
#pragma unroll
            for (int t = 0; t < 2; t++) {
                if (!((inf >> (12 + t)) & 1u)) continue;
                const int k = t == 0 ? s1 : (s1 % 8 + 1);
                const int nx2 = lx + d1(k), ny2 = ry0 + r + d2(k);
                if (nx2 < 0 || nx2 >= TS || ny2 < 0 || ny2 >= TS) tw |= 1u << (26 + t);
                else tw |= (unsigned(ny2 * TS + nx2) << (12 * t)) | (1u << (24 + t));
            }
            S.tw[(ry0 + r) * TS + lx] = tw;
            if constexpr (Dim<TSZ>::template USE_CW<HAS_DM>) {
                unsigned cw = (unsigned(__popc(inf & 0xFFu)) << 28) | ((inf & 0x100u) << 19), mm = inf & 0xFFu;
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    const int k = mm ? __ffs(int(mm)) : 0;
                    mm &= mm - 1u;
                    if (k) cw |= ((unsigned(d2(k) * LH + d1(k)) & 0xFFu) | (((inf >> (15 + k)) & 1u) << 8)) << (9 * i);
                }
                S.cw[(ry0 + r) * TS + lx] = cw;
            }
        }
        if (tid < TS) S.dx[tid] = dxrow;
    }
    __syncthreads();
    const unsigned long long tc1 = dbg ? wall_clock64() : 0ull;
    unsigned pendmask = 0;   // own cells that are pending (participating, owned by this rank, not evaluated yet)
#pragma unroll
    for (int r = 0; r < RPL; r++) {
        const int gx = x0 + lx, gy = y0 + ry0 + r;
        if (gx < g.nx && gy >= g.y_own0 && gy < g.y_own1 && pending(S.out[(ry0 + r + 1) * LH + lx + 1])) pendmask |= 1u << r;
    }
    const unsigned pend0 = pendmask;
    int rim = 0;
    // ---- bulk: a fresh tile holds thousands of ready cells and short chains - evaluated in lockstep (every lane looks at its
    // own pending cells: ready = no contributor pending), one dependency level or more per sweep, no atomics.  What is left
    // after a few sweeps are the stream cells: long, thin chains for the walks below.
    if (full) {
        for (int sweep = 0; sweep < g.max_sweeps; sweep++) {   // (TileGeom::max_sweeps carries the number of lockstep sweeps here: TDX_DINF_BULK_SWEEPS)
            bool prog = false;
#pragma unroll
            for (int rr = 0; rr < RPL; rr++) {
                const int r = (sweep & 1) ? RPL - 1 - rr : rr;
                if (!((pendmask >> r) & 1u)) continue;
                const int ly = ry0 + r, c = ly * TS + lx, cl = (ly + 1) * LH + lx + 1;
                const unsigned inf = S.info[c];
                float val;
                if (eval_cell<true, Eval, TSZ, HAS_W, HAS_DM>(ev, S, c, cl, ly, inf, contcheck, &val)) {
                    S.out[cl] = val;
                    rim |= rim_bits<TSZ>(inf, lx, ly);
                    pendmask &= ~(1u << r);
                    prog = true;
                }
            }
            if (!__syncthreads_or(prog ? 1 : 0)) break;
        }
    }
    // ---- pending contributors of the cells that are left
    unsigned readymask = 0;
    uint8_t* cnt8 = reinterpret_cast<uint8_t*>(S.cnt);
#pragma unroll
    for (int r = 0; r < RPL; r++) {
        const int ly = ry0 + r, c = ly * TS + lx, cl = (ly + 1) * LH + lx + 1;
        unsigned cn = 255u;
        const unsigned inf = S.info[c];
        float nv[9];
#pragma unroll
        for (int k = 1; k <= 8; k++) nv[k] = S.out[cl + d2(k) * LH + d1(k)];
        if ((pendmask >> r) & 1u) {
            unsigned pb = 0;
#pragma unroll
            for (int k = 1; k <= 8; k++) pb |= pending(nv[k]) ? 1u << (k - 1) : 0u;
            cn = unsigned(__popc(inf & 0xFFu & pb));
            if (cn == 0u) readymask |= 1u << r;
        }
        cnt8[c] = uint8_t(cn);
    }
    __syncthreads();
    const unsigned long long tc2 = dbg ? wall_clock64() : 0ull;
    // ---- walks: a lane follows a chain downstream as long as it finishes the last pending contributor of a target
    auto walk = [&](int c, int phase) {
        unsigned inf = S.info[c], tw = S.tw[c];
        uint32_t* const spare = &S.spare[tid & 63];
        for (;;) {
            const int ly = c / TS, cx = c % TS, cl = (ly + 1) * LH + cx + 1;
            float val;
            (void)eval_cell<false, Eval, TSZ, HAS_W, HAS_DM>(ev, S, c, cl, ly, inf, contcheck, &val);
            S.out[cl] = val;
            hops++;
            if (tw >> 26) rim |= rim_bits<TSZ>(inf, cx, ly);   // a target in a neighbouring tile (cells on the tile's rim only)
            // the (at most two) targets in the tile: both decrements and the candidates' info / target words are in flight together, without a branch
            // (a target that does not exist decrements the lane's spare word and reads cell 0; `ok` keeps it out of what follows)
            const int t0 = int(tw & 0xFFFu), t1 = int((tw >> 12) & 0xFFFu);
            const bool ok0 = ((tw >> 24) & 1u) != 0u, ok1 = ((tw >> 25) & 1u) != 0u;
            const unsigned sh0 = 8u * unsigned(t0 & 3), sh1 = 8u * unsigned(t1 & 3);
            const unsigned old0 = __hip_atomic_fetch_sub(ok0 ? &S.cnt[t0 >> 2] : spare, 1u << sh0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const unsigned old1 = __hip_atomic_fetch_sub(ok1 ? &S.cnt[t1 >> 2] : spare, 1u << sh1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const unsigned inf0 = S.info[t0], inf1 = S.info[t1], tw0 = S.tw[t0], tw1 = S.tw[t1];
            const bool last0 = ok0 && ((old0 >> sh0) & 255u) == 1u, last1 = ok1 && ((old1 >> sh1) & 255u) == 1u;   // its last pending contributor
            if (last0 && last1) {   // a fork with both branches ready: the second one goes to the queue of the next phase
                const unsigned slot = atomicAdd(&S.nq[phase ^ 1], 1u);
                if (slot < unsigned(QLEN)) S.q[phase ^ 1][slot] = uint16_t(t1);
                else S.over = 1;
            }
            if (!(last0 || last1)) break;
            c = last0 ? t0 : t1;
            inf = last0 ? inf0 : inf1;
            tw = last0 ? tw0 : tw1;
        }
    };
    for (unsigned m = readymask; m; m &= m - 1u) walk((ry0 + (__ffs(int(m)) - 1)) * TS + lx, 0);
    for (int phase = 1;; phase ^= 1) {          // drain the hand-over queue: the walks of a phase fill the other buffer
        __syncthreads();                        // every push into q[phase] has landed
        const unsigned n = S.nq[phase] < unsigned(QLEN) ? S.nq[phase] : unsigned(QLEN);
        if (n == 0u) break;
        nphase++;
        for (unsigned i = tid; i < n; i += unsigned(NT)) walk(int(S.q[phase][i]), phase);
        __syncthreads();                        // q[phase] has been read by everybody
        if (tid == 0) S.nq[phase] = 0u;         // (nobody pushes into it before the next barrier)
    }
    const unsigned long long tc3 = dbg ? wall_clock64() : 0ull;
    // ---- write back what this activation evaluated
    bool wrote = false;
    for (unsigned m = pend0; m; m &= m - 1u) {
        const int r = __ffs(int(m)) - 1, ly = ry0 + r;
        const float v = S.out[(ly + 1) * LH + lx + 1];
        if (!pending(v)) { OUT[size_t(y0 + ly) * size_t(g.nx) + size_t(x0 + lx)] = v; wrote = true; }
    }
    if (rim) atomicOr(&S.rim, rim);
    // "did anybody write" through LDS and a barrier that waits for the LDS only: __syncthreads_or() is a workgroup-scope release, i.e. it sits out
    // the acknowledgement of every global store above (5 - 7 us per activation in the phase clocks).  Nobody in this launch depends on those stores
    // having landed: a neighbour that stages its ring meanwhile sees the old or the new record (the contract of the sweeps), the next round is
    // another launch, and the solo hand-over of round_driver fences for itself.
    if (wrote) S.wrote = 1;
    tdx_barrier_lds();
    const int any = S.wrote;
    const int res = (any ? (tilek::RES_CHANGED | S.rim) : 0) | (S.over ? tilek::RES_CAPPED : 0);
    if (dbg) {   // TDX_DEBUG_ROUNDS=1: 100 MHz ticks per phase, hops (total and of the busiest lane), hand-over phases
        // accumulated in LDS (S.dbg) and flushed ONCE per workgroup and launch by sweep_kernel: the first version added to eight device counters per activation
        // - 256 lanes on one address for the hops - and the hot atomics, waited for by the NEXT activation's loads, inflated its "stage" phase tenfold
        atomicAdd(&S.nq[1], unsigned(hops));   // (the queue counters are idle here)
        atomicMax(&S.nq[0], unsigned(hops));
        {   // staged vs evaluated: of the TS x TS records an activation stages, how many were still pending, and how many did it finish
            unsigned done = 0;
            for (unsigned m = pend0; m; m &= m - 1u) done += !pending(S.out[(ry0 + (__ffs(int(m)) - 1) + 1) * LH + lx + 1]);
            atomicAdd(&S.dbg[8], (unsigned long long)__popc(pend0));
            atomicAdd(&S.dbg[9], (unsigned long long)done);
        }
        __syncthreads();
        if (tid == 0) {
            const unsigned long long tc4 = wall_clock64();
            S.dbg[0] += tc1 - tc0; S.dbg[1] += tc2 - tc1; S.dbg[2] += tc3 - tc2; S.dbg[3] += tc4 - tc3;
            S.dbg[4] += S.nq[1]; S.dbg[5] += S.nq[0]; S.dbg[6] += nphase; S.dbg[7] += 1ull;
        }
    }
    tdx_barrier_lds();   // S is reused by the next tile (the write-back's global stores drain while it is staged)
    return res;
}

template <class Eval, int TSZ, bool HAS_W, bool HAS_DM>
__global__ __launch_bounds__(Dim<TSZ>::NT) void sweep_kernel(Eval ev, tilek::TileGeom g, const uint32_t* __restrict__ list, unsigned long long* __restrict__ count,
                                                   uint32_t* __restrict__ flags_cur, uint32_t* __restrict__ flags_next, uint32_t* __restrict__ list_next,
                                                   unsigned pull_max, const double2* __restrict__ P, const float* __restrict__ W, const float* __restrict__ DM,
                                                   const uint32_t* __restrict__ INFO, const RowProp* __restrict__ rows, float* __restrict__ OUT,
                                                   float out_nodata, int contcheck, unsigned long long* __restrict__ dbg) {
    __shared__ Lds<TSZ, HAS_W, HAS_DM> S;
    __shared__ tilek::TileLds L;
    if (dbg && threadIdx.x < 10) S.dbg[threadIdx.x] = 0ull;
    tilek::round_driver(list, count, flags_cur, flags_next, list_next, pull_max, g, L, [&](int tile, bool full) {
        return sweep_tile<Eval, TSZ, HAS_W, HAS_DM>(ev, g, tile, full, S, P, W, DM, INFO, rows, OUT, out_nodata, contcheck, dbg);
    });
    if (dbg) {
        __syncthreads();
        if (threadIdx.x < 10 && S.dbg[threadIdx.x]) atomicAdd(dbg + threadIdx.x, S.dbg[threadIdx.x]);
    }
}
}  // namespace dsweep
