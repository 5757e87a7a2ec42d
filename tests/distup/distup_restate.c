/* A plain C restatement of DinfDistUp's semantics (dinfdistup, src/DinfDistUp.cpp), written from the rules of DESIGN.md section
 * "DinfDistUp": one FIFO queue over the whole raster (Kahn's algorithm over the neighbours that drain into a cell), the D-infinity
 * proportions from prop(), float accumulators with double proportions.  It is the checker at sizes the reference goldens do not
 * cover; its own CPU test holds it to every golden bit for bit.  Built by the tests with `cc -O2 -ffp-contract=off -shared -fPIC`
 * (x86-64: SSE arithmetic, no contraction - the rounding of the reference build).
 *
 * kind: 0 h, 1 v, 2 p, 3 s; stat: 0 ave, 1 max, 2 min.  fel may be NULL for h, w may be NULL (no weights).  thresh: a contributor
 * counts only if p > thresh.  out: float, -FLT_MAX where there is no result.  Returns 0, or -1 when memory runs out. */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#define PI_ 3.14159265359
#define EPS_ 1E-5f
static const int DX_[9] = {0, 1, 1, 0, -1, -1, -1, 0, 1};
static const int DY_[9] = {0, 0, -1, -1, -1, 0, 1, 1, 1};

static int nodata_f(float v, float nd) { return fabsf((float)(v - nd)) < EPS_; }

/* the share of the flow of a cell with angle a that goes to neighbour k (k = 0 means 8); 0 or less: none */
static double prop_(float a, int k, double dx, double dy) {
    const double a0 = atan2(dy, dx);
    const double aref[10] = {-a0, 0., a0, 0.5 * PI_, PI_ - a0, PI_, PI_ + a0, 1.5 * PI_, 2. * PI_ - a0, 2. * PI_};
    double p = 0.;
    if (k <= 0) k += 8;
    if (k == 1 && a > PI_) a = (float)(a - 2.0 * PI_);
    if (a > aref[k - 1] && a < aref[k + 1]) {
        if (a > aref[k]) p = (aref[k + 1] - a) / (aref[k + 1] - aref[k]);
        else p = (a - aref[k - 1]) / (aref[k] - aref[k - 1]);
    }
    return p < 1e-5 ? -1. : p;
}

int distup(int nx, int ny, const float* ang, float ang_nd, const float* fel, float fel_nd, const float* w, float w_nd, const double* dxc, const double* dyc,
           int stat, int kind, int concheck, float thresh, float* out) {
    const float ND = -FLT_MAX;
    const size_t n = (size_t)nx * (size_t)ny;
    const int use_w = w != NULL && kind != 1;
    float* dh = out;                                          /* h / v / s result, or the h part of p */
    float* dv = kind == 2 ? malloc(n * sizeof(float)) : NULL; /* the v part of p */
    int* waiting = malloc(n * sizeof(int));                   /* contributors not finished yet */
    size_t* queue = malloc(n * sizeof(size_t));
    float* dist = malloc((size_t)ny * 9 * sizeof(float));
    if ((kind == 2 && !dv) || !waiting || !queue || !dist) { free(dv); free(waiting); free(queue); free(dist); return -1; }
    for (int j = 0; j < ny; j++)
        for (int k = 1; k <= 8; k++) dist[(size_t)j * 9 + k] = (float)sqrt(dxc[j] * dxc[j] * DX_[k] * DX_[k] + dyc[j] * dyc[j] * DY_[k] * DY_[k]);
    size_t head = 0, tail = 0;
    for (size_t c = 0; c < n; c++) { dh[c] = ND; if (dv) dv[c] = ND; waiting[c] = 0; }
    /* in-degree: neighbours inside the raster with an angle whose flow reaches the cell (thresh plays no part here) */
    for (int j = 0; j < ny; j++)
        for (int i = 0; i < nx; i++) {
            const size_t c = (size_t)j * nx + i;
            if (nodata_f(ang[c], ang_nd)) continue;
            int cnt = 0;
            for (int k = 1; k <= 8; k++) {
                const int in = i + DX_[k], jn = j + DY_[k];
                if (in < 0 || in >= nx || jn < 0 || jn >= ny) continue;
                const size_t cn = (size_t)jn * nx + in;
                if (!nodata_f(ang[cn], ang_nd) && prop_(ang[cn], (k + 4) % 8, dxc[jn], dyc[jn]) > 0.) cnt++;
            }
            waiting[c] = cnt;
            if (cnt == 0) queue[tail++] = c;
        }
    while (head < tail) {
        const size_t c = queue[head++];
        const int i = (int)(c % (size_t)nx), j = (int)(c / (size_t)nx);
        if ((kind == 2 || kind == 3) && nodata_f(fel[c], fel_nd)) { dh[c] = ND; if (dv) dv[c] = ND; }   /* v has no such test */
        else {
            int con = 0, first = 1;
            float sump = 0.f, acc = 0.f, accv = 0.f;
            const float elv = kind != 0 ? fel[c] : 0.f;   /* v: the raw value, nodata or not */
            for (int k = 1; k <= 8; k++) {
                const int in = i + DX_[k], jn = j + DY_[k];
                if (in < 0 || in >= nx || jn < 0 || jn >= ny) { con = 1; continue; }
                const size_t cn = (size_t)jn * nx + in;
                if (nodata_f(ang[cn], ang_nd)) { con = 1; continue; }
                const double p = prop_(ang[cn], (k + 4) % 8, dxc[jn], dyc[jn]);   /* the contributor's row */
                if (!(p > 0. && p > thresh)) continue;
                if (nodata_f(dh[cn], ND)) { con = 1; continue; }
                if (kind != 0 && nodata_f(fel[cn], fel_nd)) { con = 1; continue; }
                sump = sump + p;
                float wt = 1.f;
                if (use_w) {
                    if (nodata_f(w[cn], w_nd)) con = 1;
                    else wt = w[cn];
                }
                float x, xv = 0.f;
                const float dk = dist[(size_t)j * 9 + k] * wt;   /* the row of the evaluated cell */
                if (kind == 0) x = dk + dh[cn];
                else if (kind == 1) x = (fel[cn] - elv) + dh[cn];
                else if (kind == 2) { x = dk + dh[cn]; xv = (fel[cn] - elv) + dv[cn]; }
                else { const float dz = elv - fel[cn]; x = sqrtf(dz * dz + dk * dk) + dh[cn]; }
                if (stat == 0) {
                    acc = acc + p * x;
                    accv = accv + p * xv;
                } else if (stat == 1 && kind == 0) {
                    if (x > acc) acc = x;   /* max h starts from 0 */
                } else if (first) {
                    acc = x; accv = xv; first = 0;
                } else if (stat == 1) {
                    if (x > acc) acc = x;
                    if (xv > accv) accv = xv;
                } else {
                    if (x < acc) acc = x;
                    if (xv < accv) accv = xv;
                }
            }
            if (con && concheck) { dh[c] = ND; if (dv) dv[c] = ND; }
            else if (stat == 0 && sump > 0.) { dh[c] = acc / sump; if (dv) dv[c] = accv / sump; }
            else { dh[c] = acc; if (dv) dv[c] = accv; }
        }
        /* release the (at most two) receivers */
        for (int k = 1; k <= 8; k++) {
            const int in = i + DX_[k], jn = j + DY_[k];
            if (in < 0 || in >= nx || jn < 0 || jn >= ny) continue;
            const size_t cn = (size_t)jn * nx + in;
            if (nodata_f(ang[cn], ang_nd)) continue;
            if (prop_(ang[c], k, dxc[j], dyc[j]) > 0.) {
                if (--waiting[cn] == 0) queue[tail++] = cn;
            }
        }
    }
    if (kind == 2)   /* sqrt(h^2 + v^2) where both are known */
        for (size_t c = 0; c < n; c++) {
            if (nodata_f(dv[c], ND)) dh[c] = ND;
            else if (!nodata_f(dh[c], ND)) dh[c] = sqrtf(dh[c] * dh[c] + dv[c] * dv[c]);
        }
    free(dv); free(waiting); free(queue); free(dist);
    return 0;
}
