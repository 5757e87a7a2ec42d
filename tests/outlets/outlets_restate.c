/* MoveOutletsToStrm and ConnectDown as plain C on whole rasters, one rank: the loops of src/MoveOutletsToStrm.cpp:370-435 and of
 * src/ConnectDown.cpp:177-247, :318-340, :402-434, written out as the reference has them (arrays indexed by id, one pass over the outlets per
 * round, a strict > for the maximum).  tests/test_outlets_restatement.py holds it to the goldens of the real tools, so that the GPU tests can use
 * it at sizes the goldens do not cover.  The *_rows / *_step functions are the same loops on a band of rows: the CPU model of the hand-over
 * between row strips (tests/outlets_model.py).  src is int32 here as in the library (the reference reads it as int16; the values are the same). */
#include <stdint.h>
#include <stdlib.h>

static const int d1[9] = {-99, 0, -1, -1, -1, 0, 1, 1, 1};   /* row step */
static const int d2[9] = {-99, 1, 1, 0, -1, -1, -1, 0, 1};   /* column step */

#define AT(g, x, y) (g)[(size_t)(y) * (size_t)nx + (size_t)(x)]

/* columns x / rows y in and out; dist out (-1: not moved).  Rows [own0, own1) are "the partition": one rank has own0 = 0, own1 = ny.
 * is_done: 1 not done, 0 done, as the reference counts.  Returns the number of outlets that are not done. */
static long move_round(int nx, int ny, const int16_t* p, int16_t p_nodata, const int32_t* src, int32_t src_nodata, int maxdist, int own0, int own1, long n, int32_t* ox,
                       int32_t* oy, int32_t* dist_moved, int32_t* is_done, long* touched) {
    long done = 0, i;
    const int itresh = 1;
    for (i = 0; i < n; i++) {
        int tx = ox[i], ty = oy[i];
        while (tx >= 0 && tx < nx && ty >= own0 && ty < own1 && is_done[i] != 0) {
            int32_t td;
            if (touched) touched[0]++;
            if (AT(p, tx, ty) == p_nodata) is_done[i] = 0;
            td = AT(src, tx, ty);
            if (td == src_nodata || td < itresh) {
                const int16_t dirn = AT(p, tx, ty);
                if (dirn >= 1 && dirn <= 8 && dist_moved[i] < maxdist) {
                    const int nextx = ox[i] + d2[dirn], nexty = oy[i] + d1[dirn];
                    if (nextx >= 0 && nexty >= 0 && nextx < nx && nexty < ny) { ox[i] = nextx; oy[i] = nexty; dist_moved[i]++; }
                    else { dist_moved[i] = -1; is_done[i] = 0; }
                } else { dist_moved[i] = -1; is_done[i] = 0; }
            } else is_done[i] = 0;
            tx = ox[i]; ty = oy[i];
        }
        done += is_done[i];
    }
    return done;
}

int or_moveoutlets(int nx, int ny, const int16_t* p, int16_t p_nodata, const int32_t* src, int32_t src_nodata, int maxdist, long n, int32_t* ox, int32_t* oy,
                   int32_t* dist_moved) {
    int32_t* is_done = (int32_t*)malloc(sizeof(int32_t) * (size_t)(n > 0 ? n : 1));
    long i, done = 0;
    if (!is_done) return 1;
    for (i = 0; i < n; i++) {
        dist_moved[i] = 0; is_done[i] = 1;
        if (ox[i] < 0 || ox[i] >= nx || oy[i] < 0 || oy[i] >= ny) { is_done[i] = 0; dist_moved[i] = -1; }
        done += is_done[i];
    }
    while (done > 0) done = move_round(nx, ny, p, p_nodata, src, src_nodata, maxdist, 0, ny, n, ox, oy, dist_moved, is_done, NULL);
    free(is_done);
    return 0;
}

/* one strip's turn: state_done is 0 / 1 = not done / done (the library's sense); returns the iterations made */
long or_moveoutlets_step(int nx, int ny, const int16_t* p, int16_t p_nodata, const int32_t* src, int32_t src_nodata, int maxdist, int own0, int own1, long n,
                         int32_t* ox, int32_t* oy, int32_t* dist_moved, int32_t* state_done) {
    long i, touched = 0;
    for (i = 0; i < n; i++) {
        if (!state_done[i] && (ox[i] < 0 || ox[i] >= nx || oy[i] < 0 || oy[i] >= ny)) { state_done[i] = 1; dist_moved[i] = -1; touched++; }
        state_done[i] = !state_done[i];
    }
    move_round(nx, ny, p, p_nodata, src, src_nodata, maxdist, own0, own1, n, ox, oy, dist_moved, state_done, &touched);
    for (i = 0; i < n; i++) state_done[i] = !state_done[i];
    return touched;
}

/* The maximum of every watershed in rows [row0, row1): arrays indexed by id, 0 .. maxall - 1 (the caller sizes them by the largest id of the whole
 * raster).  Returns the count; ids / x / y (global) / ad8max of the ids found, ascending.  -1: an id outside 0 .. maxall - 1. */
long or_argmax_rows(int nx, int row0, int row1, const int32_t* w, int32_t w_nodata, const float* ad8, long maxall, int32_t* ids, int32_t* x, int32_t* y, float* ad8max) {
    int* wfound = (int*)calloc((size_t)maxall, sizeof(int));
    int32_t *wi = (int32_t*)malloc(sizeof(int32_t) * (size_t)maxall), *wj = (int32_t*)malloc(sizeof(int32_t) * (size_t)maxall);
    float* amax = (float*)calloc((size_t)maxall, sizeof(float));
    long nxy = 0, ii;
    int i, j;
    if (!wfound || !wi || !wj || !amax) return -2;
    for (j = row0; j < row1; j++)
        for (i = 0; i < nx; i++)
            if (AT(w, i, j) != w_nodata) {
                const int32_t id = AT(w, i, j);
                const float tempFloat = AT(ad8, i, j);
                if (id < 0 || id >= maxall) { nxy = -1; goto out; }
                if (wfound[id] == 0) { wfound[id] = 1; wi[id] = i; wj[id] = j; amax[id] = tempFloat; }
                else if (tempFloat > amax[id]) { wi[id] = i; wj[id] = j; amax[id] = tempFloat; }
            }
    for (ii = 0; ii < maxall; ii++)
        if (wfound[ii] > 0) { ids[nxy] = (int32_t)ii; x[nxy] = wi[ii]; y[nxy] = wj[ii]; ad8max[nxy] = amax[ii]; nxy++; }
out:
    free(wfound); free(wi); free(wj); free(amax);
    return nxy;
}

/* largest id (0 when there is none: "this assumes that the maximum will be positive") and smallest id (INT32_MAX when there is none) */
void or_id_range(int nx, int ny, const int32_t* w, int32_t w_nodata, int32_t* wmax, int32_t* wmin) {
    int i, j;
    *wmax = 0; *wmin = INT32_MAX;
    for (j = 0; j < ny; j++)
        for (i = 0; i < nx; i++)
            if (AT(w, i, j) != w_nodata) {
                if (AT(w, i, j) > *wmax) *wmax = AT(w, i, j);
                if (AT(w, i, j) < *wmin) *wmin = AT(w, i, j);
            }
}

/* One round of the walk over every point that lies in rows [own0, own1) with dist_moved >= 0 (src/ConnectDown.cpp:406-434); returns how many moved
 * or stopped.  A point stops with dist_moved = -1 and stays where it is. */
long or_walkdown_round(int nx, int ny, const int16_t* p, const int32_t* w, int movedist, int own0, int own1, long n, int32_t* ox, int32_t* oy, int32_t* dist_moved,
                       int32_t* widdown) {
    long i, active = 0;
    for (i = 0; i < n; i++) {
        const int tx = ox[i], ty = oy[i];
        if (ty >= own0 && ty < own1 && dist_moved[i] >= 0) {
            const int16_t dirn = AT(p, tx, ty);
            active++;
            widdown[i] = AT(w, tx, ty);
            if (dirn >= 1 && dirn <= 8 && dist_moved[i] < movedist) {
                const int nextx = ox[i] + d2[dirn], nexty = oy[i] + d1[dirn];
                if (nextx >= 0 && nexty >= 0 && nextx < nx && nexty < ny) {
                    ox[i] = nextx; oy[i] = nexty; dist_moved[i]++;
                    if (nexty >= own0 && nexty < own1) widdown[i] = AT(w, nextx, nexty);   /* (a strip reads its own rows only; the next owner sets it again) */
                } else dist_moved[i] = -1;
            } else dist_moved[i] = -1;
        }
    }
    return active;
}

/* ConnectDown on one rank.  Returns the count, -1 for an id that is negative or above cap. */
long or_connectdown(int nx, int ny, const int16_t* p, const int32_t* w, int32_t w_nodata, const float* ad8, int movedist, long cap, int32_t* ids, int32_t* x, int32_t* y,
                    float* ad8max, int32_t* mx, int32_t* my, int32_t* widdown) {
    int32_t wmax, wmin;
    long nxy, i;
    int32_t* dist_moved;
    or_id_range(nx, ny, w, w_nodata, &wmax, &wmin);
    if (wmin < 0 || wmax > cap) return -1;
    nxy = or_argmax_rows(nx, 0, ny, w, w_nodata, ad8, (long)wmax + 1, ids, x, y, ad8max);
    if (nxy <= 0) return nxy;
    dist_moved = (int32_t*)calloc((size_t)nxy, sizeof(int32_t));
    if (!dist_moved) return -2;
    for (i = 0; i < nxy; i++) { mx[i] = x[i]; my[i] = y[i]; widdown[i] = 0; }
    while (or_walkdown_round(nx, ny, p, w, movedist, 0, ny, nxy, mx, my, dist_moved, widdown) > 0) {}
    free(dist_moved);
    return nxy;
}
