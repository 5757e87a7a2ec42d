/* A plain C restatement of D8HDistToStrm (distgrid, src/D8HDistToStrm.cpp) and GageWatershed (gagewatershed, src/gagewatershed.cpp),
 * written from the rules of DESIGN.md section "D8HDistToStrm and GageWatershed": one FIFO queue over the whole raster (Kahn's
 * algorithm) that starts at the sources and walks upstream.  It is the checker at sizes the reference goldens do not cover; its own CPU
 * test holds it to every golden bit for bit and to every -id file byte for byte.  Built by the tests with `cc -O2 -ffp-contract=off
 * -shared -fPIC`.  Returns 0, or -1 when memory runs out. */
#include <float.h>
#include <stdint.h>
#include <stdlib.h>
#include <math.h>

static const int DX_[9] = {0, 1, 1, 0, -1, -1, -1, 0, 1};
static const int DY_[9] = {0, 0, -1, -1, -1, 0, 1, 1, 1};
#define GW_ND (-2147483647)

/* dist: -FLT_MAX where there is no result.  Stream: src != src_nd and src >= thresh, whatever p is. */
int d8hdist(int nx, int ny, const int16_t* p, int16_t p_nd, const int32_t* src, int32_t src_nd, int32_t thresh, const double* dxc, const double* dyc,
            float* out) {
    const float ND = -FLT_MAX;
    const size_t n = (size_t)nx * (size_t)ny;
    int* waiting = malloc(n * sizeof(int));   /* the reference's `neighbor`: 1 with a direction, 0 for stream cells, INT_MIN for neither */
    size_t* queue = malloc(n * sizeof(size_t));
    float* dist = malloc((size_t)ny * 9 * sizeof(float));
    if (!waiting || !queue || !dist) { free(waiting); free(queue); free(dist); return -1; }
    for (int j = 0; j < ny; j++)
        for (int k = 1; k <= 8; k++) dist[(size_t)j * 9 + k] = (float)sqrt(DX_[k] * DX_[k] * dxc[j] * dxc[j] + DY_[k] * DY_[k] * dyc[j] * dyc[j]);
    size_t head = 0, tail = 0;
    for (size_t c = 0; c < n; c++) {
        out[c] = ND;
        waiting[c] = p[c] != p_nd ? 1 : -2147483647 - 1;
        if (src[c] != src_nd && src[c] >= thresh) { waiting[c] = 0; queue[tail++] = c; }
    }
    while (head < tail) {
        const size_t c = queue[head++];
        const int i = (int)(c % (size_t)nx), j = (int)(c / (size_t)nx);
        if (src[c] != src_nd && src[c] >= thresh) out[c] = 0.0f;
        else {
            const int k = p[c];   /* a released cell has a direction; p == 0 reads the cell itself (still nodata) */
            if (k >= 0 && k <= 8) {
                const int in = i + DX_[k], jn = j + DY_[k];
                if (in >= 0 && in < nx && jn >= 0 && jn < ny) {
                    const float v = out[(size_t)jn * nx + in];
                    out[c] = v == ND ? ND : (float)(dist[(size_t)j * 9 + k] + v);
                }
            }
        }
        for (int k = 1; k <= 8; k++) {   /* upstream: neighbours whose code points back, any sign */
            const int in = i + DX_[k], jn = j + DY_[k];
            if (in < 0 || in >= nx || jn < 0 || jn >= ny) continue;
            const size_t m = (size_t)jn * nx + in;
            if (p[m] == p_nd) continue;
            if (p[m] - k == 4 || p[m] - k == -4) {
                if (--waiting[m] == 0) queue[tail++] = m;
            }
        }
    }
    free(waiting); free(queue); free(dist);
    return 0;
}

/* gw: MISSINGLONG where unreached.  Outlets: global column / row, ids; towrite[i] = 1 where outlet i labels its cell (the first on a cell,
 * inside the raster); dsids[i]: the -id file's iddown column. */
int gagews(int nx, int ny, const int16_t* p, int16_t p_nd, int nout, const int32_t* ox, const int32_t* oy, const int32_t* ids, int32_t* gw,
           int32_t* towrite, int32_t* dsids) {
    const size_t n = (size_t)nx * (size_t)ny;
    int* waiting = malloc(n * sizeof(int));
    size_t* queue = malloc((n + (size_t)nout + 1) * sizeof(size_t));
    if (!waiting || !queue) { free(waiting); free(queue); return -1; }
    size_t head = 0, tail = 0;
    for (size_t c = 0; c < n; c++) { gw[c] = GW_ND; waiting[c] = p[c] != p_nd ? 1 : -32768; }
    for (int o = 0; o < nout; o++) {
        towrite[o] = 0;
        dsids[o] = -1;
        if (ox[o] < 0 || ox[o] >= nx || oy[o] < 0 || oy[o] >= ny) continue;
        const size_t c = (size_t)oy[o] * nx + ox[o];
        if (gw[c] != GW_ND) continue;
        gw[c] = ids[o];
        queue[tail++] = c;
        towrite[o] = 1;
    }
    while (head < tail) {
        const size_t c = queue[head++];
        const int i = (int)(c % (size_t)nx), j = (int)(c / (size_t)nx);
        if (gw[c] == GW_ND) {   /* released: label of the receiver */
            const int k = p[c];
            gw[c] = gw[(size_t)(j + DY_[k]) * nx + (i + DX_[k])];
        }
        for (int k = 1; k <= 8; k++) {
            const int in = i + DX_[k], jn = j + DY_[k];
            if (in < 0 || in >= nx || jn < 0 || jn >= ny) continue;
            const size_t m = (size_t)jn * nx + in;
            const int sdir = p[m];
            if (sdir <= 0 || (sdir - k != 4 && sdir - k != -4)) continue;
            if (sdir != p_nd && gw[m] == GW_ND) {
                if (--waiting[m] == 0) queue[tail++] = m;
            }
            if (gw[m] != GW_ND) {   /* an upstream gauge: its id's entry gets this cell's label */
                int x = 0;
                while (x < nout && ids[x] != gw[m]) x++;
                if (x < nout) dsids[x] = gw[c];
            }
        }
    }
    free(waiting); free(queue);
    return 0;
}
