/* A plain C restatement of FlowDirCond (flowdircond, src/flowdircond.cpp), D8VDistToStrm (d8vdistdown, src/D8VDistToStrm.cpp) and
 * SlopeAveDown (sloped, src/SlopeAveDown.cpp), written from the rules of DESIGN.md section "FlowDirCond, D8VDistToStrm and SlopeAveDown":
 * one FIFO queue over the whole raster (Kahn's algorithm), SlopeAveDown with one full queue pass per iteration that updates ed / dd IN
 * PLACE, as the reference does - not the double-buffered pull of the GPU kernel, which it is there to check.  It is the checker at sizes
 * the reference goldens do not cover; its own CPU test holds it to every golden bit for bit.  Built by the tests with `cc -O2
 * -ffp-contract=off -shared -fPIC`.  Every function returns 0, or -1 when memory runs out. */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static const int DX_[9] = {0, 1, 1, 0, -1, -1, -1, 0, 1};
static const int DY_[9] = {0, 0, -1, -1, -1, 0, 1, 1, 1};
#define ND (-FLT_MAX)
#define NOT_PART (-32768)

/* linearpart<float>::isNodata (src/linearpart.h:476) */
static int nodata_f(float v, float nd) { return fabsf((float)(v - nd)) < 1e-5f; }

/* initNeighborD8up without outlets (src/commonLib.cpp:251-282): a cell takes part where p is 0..8; its count is the number of neighbours
 * with a code 0..8 and code - k == +-4 (a p == 0 neighbour counts at k == 4); cells with count 0 start the queue.  Returns the tail. */
static size_t init_queue(int nx, int ny, const int16_t* p, int16_t p_nd, int* waiting, size_t* queue) {
    size_t tail = 0;
    for (int j = 0; j < ny; j++)
        for (int i = 0; i < nx; i++) {
            const size_t c = (size_t)j * nx + i;
            waiting[c] = NOT_PART;
            if (p[c] == p_nd || p[c] < 0 || p[c] > 8) continue;
            int cnt = 0;
            for (int k = 1; k <= 8; k++) {
                const int in = i + DX_[k], jn = j + DY_[k];
                if (in < 0 || in >= nx || jn < 0 || jn >= ny) continue;
                const int16_t q = p[(size_t)jn * nx + in];
                if (q == p_nd || q < 0 || q > 8) continue;
                if (q - k == 4 || q - k == -4) cnt++;
            }
            waiting[c] = cnt;
            if (cnt == 0) queue[tail++] = c;
        }
    return tail;
}

/* src/flowdircond.cpp:143-194.  out: z with the popped cells lowered. */
int flowdircond(int nx, int ny, const int16_t* p, int16_t p_nd, const float* z, float z_nd, float* out) {
    const size_t n = (size_t)nx * (size_t)ny;
    int* waiting = malloc(n * sizeof(int));
    size_t* queue = malloc(n * sizeof(size_t));
    if (!waiting || !queue) { free(waiting); free(queue); return -1; }
    memcpy(out, z, n * sizeof(float));
    size_t head = 0, tail = init_queue(nx, ny, p, p_nd, waiting, queue);
    while (head < tail) {
        const size_t c = queue[head++];
        const int i = (int)(c % (size_t)nx), j = (int)(c / (size_t)nx);
        if (!nodata_f(out[c], z_nd)) {   /* :151-172 */
            float zval = out[c];
            for (int k = 1; k <= 8; k++) {
                const int in = i + DX_[k], jn = j + DY_[k];
                if (in < 0 || in >= nx || jn < 0 || jn >= ny) continue;
                const size_t m = (size_t)jn * nx + in;
                const int sdir = p[m];
                if (sdir < 1 || sdir > 8 || nodata_f(out[m], z_nd)) continue;
                if (out[m] < zval && (sdir - k == 4 || sdir - k == -4)) { zval = out[m]; out[c] = zval; }
            }
        }
        const int k = p[c];   /* :175-193: a popped cell has a code 0..8; k == 0 points at the cell itself, whose count never reaches 0 again */
        const int in = i + DX_[k], jn = j + DY_[k];
        if (k >= 1 && in >= 0 && in < nx && jn >= 0 && jn < ny) {
            const size_t m = (size_t)jn * nx + in;
            if (p[m] != p_nd && p[m] >= 0 && p[m] <= 8 && --waiting[m] == 0) queue[tail++] = m;
        }
    }
    free(waiting); free(queue);
    return 0;
}

/* src/D8VDistToStrm.cpp:153-219.  out: -FLT_MAX where there is no result.  Stream: src != src_nd and src >= thresh, whatever p is. */
int d8vdist(int nx, int ny, const int16_t* p, int16_t p_nd, const float* fel, const int32_t* src, int32_t src_nd, int32_t thresh, float* out) {
    const size_t n = (size_t)nx * (size_t)ny;
    int* waiting = malloc(n * sizeof(int));
    size_t* queue = malloc(n * sizeof(size_t));
    if (!waiting || !queue) { free(waiting); free(queue); return -1; }
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
                    const size_t m = (size_t)jn * nx + in;
                    const float drop = fel[c] - fel[m];   /* no nodata test (:191-198) */
                    out[c] = out[m] == ND ? ND : (float)(drop + out[m]);
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
    free(waiting); free(queue);
    return 0;
}

/* src/SlopeAveDown.cpp:119-296.  niter full queue passes; ed / dd are updated in place while the queue runs.  out (sd): -FLT_MAX where
 * no slope was set. */
int slopeavedown(int nx, int ny, const int16_t* p, int16_t p_nd, const float* z, float z_nd, const double* dxc, const double* dyc, double dn, long niter,
                 float* out) {
    const size_t n = (size_t)nx * (size_t)ny;
    int* waiting = malloc(n * sizeof(int));
    size_t* queue = malloc(n * sizeof(size_t));
    float* ed = malloc(n * sizeof(float));
    float* dd = malloc(n * sizeof(float));
    float* dist = malloc((size_t)ny * 9 * sizeof(float));
    if (!waiting || !queue || !ed || !dd || !dist) { free(waiting); free(queue); free(ed); free(dd); free(dist); return -1; }
    for (int j = 0; j < ny; j++)
        for (int k = 1; k <= 8; k++) dist[(size_t)j * 9 + k] = (float)sqrt(DX_[k] * DX_[k] * dxc[j] * dxc[j] + DY_[k] * DY_[k] * dyc[j] * dyc[j]);
    for (size_t c = 0; c < n; c++) {   /* :153-163 */
        const int both = !nodata_f(z[c], z_nd) && p[c] != p_nd;
        ed[c] = both ? z[c] : ND;
        dd[c] = both ? 0.0f : ND;
        out[c] = ND;
    }
    for (long iter = 0; iter < niter; iter++) {
        size_t head = 0, tail = init_queue(nx, ny, p, p_nd, waiting, queue);
        while (head < tail) {
            const size_t c = queue[head++];
            const int i = (int)(c % (size_t)nx), j = (int)(c / (size_t)nx);
            const int k = p[c];
            if (k < 1 || k > 8) continue;   /* :230, 262: p == 0 only warns */
            const int in = i + DX_[k], jn = j + DY_[k];
            if (in < 0 || in >= nx || jn < 0 || jn >= ny) continue;
            const size_t m = (size_t)jn * nx + in;
            if (!nodata_f(ed[m], ND)) {   /* :234-249 */
                const float ddi = dist[(size_t)j * 9 + k] + dd[m];
                const float zi = ed[m];
                if (nodata_f(out[c], ND) && ddi > dn) out[c] = (z[c] - zi) / ddi;
                ed[c] = zi;
                dd[c] = ddi;
            }
            if (p[m] != p_nd && --waiting[m] == 0) queue[tail++] = m;   /* :251-259 (no range test on the receiver's code) */
        }
    }
    free(waiting); free(queue); free(ed); free(dd); free(dist);
    return 0;
}
