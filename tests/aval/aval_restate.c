/* A plain C restatement of RetLimFlow (retlimro, src/RetlimFlow.cpp) and DinfAvalanche (avalancherunoutgrd, src/DinfAvalanche.cpp),
 * written from the rules of DESIGN.md section 4 "RetLimFlow and DinfAvalanche": one FIFO queue over the whole raster (Kahn's algorithm
 * over the neighbours that drain into a cell), the D-infinity proportions from prop().  It keeps the REFERENCE's form - a RetLimFlow
 * cell whose wg or rc is nodata is popped, not evaluated and releases nobody, so the queue stalls below it - while the GPU evaluates
 * such a cell to nodata; the tests hold the two equal.  It is the checker at sizes the reference goldens do not cover; its own CPU test
 * holds it to every golden.  Built by the tests with `cc -O2 -ffp-contract=off -shared -fPIC` (x86-64: SSE arithmetic, no contraction -
 * the rounding of the reference build).  Results float, -FLT_MAX where there is none.  Both return 0, or -1 when memory runs out. */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define PI_ 3.14159265359
#define EPS_ 1E-5f
static const int DX_[9] = {0, 1, 1, 0, -1, -1, -1, 0, 1};
static const int DY_[9] = {0, 0, -1, -1, -1, 0, 1, 1, 1};
static const double ELIPA_ = 6378137.000, ELIPB_ = 6356752.314;

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

/* in-degrees (cells with an angle: neighbours inside the raster with an angle whose `float p` is positive; -1: no angle) and the
 * queue of the cells nobody drains into */
static void init_queue(int nx, int ny, const float* ang, float ang_nd, const double* dxc, const double* dyc, int* waiting, size_t* queue, size_t* tail) {
    for (int j = 0; j < ny; j++)
        for (int i = 0; i < nx; i++) {
            const size_t c = (size_t)j * nx + i;
            waiting[c] = -1;
            if (nodata_f(ang[c], ang_nd)) continue;
            int cnt = 0;
            for (int k = 1; k <= 8; k++) {
                const int in = i + DX_[k], jn = j + DY_[k];
                if (in < 0 || in >= nx || jn < 0 || jn >= ny) continue;
                const size_t cn = (size_t)jn * nx + in;
                if (!nodata_f(ang[cn], ang_nd) && (float)prop_(ang[cn], (k + 4) % 8, dxc[jn], dyc[jn]) > 0.0) cnt++;
            }
            waiting[c] = cnt;
            if (cnt == 0) queue[(*tail)++] = c;
        }
}
/* a finished cell releases the neighbours it sends flow to (the decrement reaches cells without an angle too; they are never queued) */
static void release(int nx, int ny, const float* ang, const double* dxc, const double* dyc, int i, int j, int* waiting, size_t* queue, size_t* tail) {
    const size_t c = (size_t)j * nx + i;
    for (int k = 1; k <= 8; k++) {
        if (!((float)prop_(ang[c], k, dxc[j], dyc[j]) > 0.0)) continue;
        const int in = i + DX_[k], jn = j + DY_[k];
        if (in < 0 || in >= nx || jn < 0 || jn >= ny) continue;
        const size_t cn = (size_t)jn * nx + in;
        if (waiting[cn] < 0) continue;
        if (--waiting[cn] == 0) queue[(*tail)++] = cn;
    }
}

int retlimflow(int nx, int ny, const float* ang, float ang_nd, const float* wg, float wg_nd, const float* rc, float rc_nd, const double* dxc, const double* dyc,
               float* qrl) {
    const size_t n = (size_t)nx * (size_t)ny;
    int* waiting = malloc(n * sizeof(int));
    size_t* queue = malloc(n * sizeof(size_t));
    if (!waiting || !queue) { free(waiting); free(queue); return -1; }
    size_t head = 0, tail = 0;
    for (size_t c = 0; c < n; c++) qrl[c] = -FLT_MAX;
    init_queue(nx, ny, ang, ang_nd, dxc, dyc, waiting, queue, &tail);
    while (head < tail) {
        const size_t c = queue[head++];
        const int i = (int)(c % (size_t)nx), j = (int)(c / (size_t)nx);
        if (nodata_f(wg[c], wg_nd) || nodata_f(rc[c], rc_nd)) continue;   /* not evaluated, releases nobody */
        float q = 0.f;
        for (int k = 1; k <= 8; k++) {   /* every neighbour inside the raster, with or without an angle */
            const int in = i + DX_[k], jn = j + DY_[k];
            if (in < 0 || in >= nx || jn < 0 || jn >= ny) continue;
            const size_t cn = (size_t)jn * nx + in;
            const float p = (float)prop_(ang[cn], (k + 4) % 8, dxc[jn], dyc[jn]);
            if (p > 0.) q = q + p * qrl[cn];
        }
        q = q + wg[c] - rc[c];
        if (q < 0.) q = 0.f;
        qrl[c] = q;
        release(nx, ny, ang, dxc, dyc, i, j, waiting, queue, &tail);
    }
    free(waiting); free(queue);
    return 0;
}

/* distance in float ulps (a large number across a NaN) */
static int64_t ulps_(float a, float b) {
    int32_t ia, ib;
    if (isnan(a) || isnan(b)) return INT64_MAX;
    memcpy(&ia, &a, 4); memcpy(&ib, &b, 4);
    const int64_t oa = ia < 0 ? (int64_t)INT32_MIN - ia : ia, ob = ib < 0 ? (int64_t)INT32_MIN - ib : ib;
    return oa > ob ? oa - ob : ob - oa;
}

/* geo = {xleftedge, ytopedge, dlon, dlat} of the raster (read in -direct mode only).  taint (may be NULL): 1 where one of the cell's
 * decisions - rz_contributor >= alpha, beta >= alpha, beta > rz so far - would flip if a computed angle moved by `tol` float ulps AND
 * the flip could change the cell's record, or where a contributor it considered is tainted.  alpha itself and a source's own rz = alpha
 * are exact; two betas compared with each other can each be off, hence 2 * tol there; two candidates with the same source, the same
 * source elevation and the same distance are the same record, whichever wins. */
int dinfavalanche(int nx, int ny, const float* ang, float ang_nd, const float* fel, float fel_nd, const int16_t* ass, int16_t ass_nd, const double* dxc,
                  const double* dyc, float thresh, float alpha, int path, const double* geo, int geographic, int tol, float* rz, float* dfs, uint8_t* taint) {
    const size_t n = (size_t)nx * (size_t)ny;
    int* waiting = malloc(n * sizeof(int));
    size_t* queue = malloc(n * sizeof(size_t));
    float* zm = malloc(n * sizeof(float));
    int32_t* im = malloc(n * sizeof(int32_t));
    int32_t* jm = malloc(n * sizeof(int32_t));
    uint8_t* isbeta = calloc(n, 1);   /* the cell's rz is a computed beta (not the exact alpha of a source) */
    float* dist = malloc((size_t)ny * 9 * sizeof(float));
    float* xcoord = malloc((size_t)nx * sizeof(float));
    float* ycoord = malloc((size_t)ny * sizeof(float));
    if (!waiting || !queue || !zm || !im || !jm || !isbeta || !dist || !xcoord || !ycoord) {
        free(waiting); free(queue); free(zm); free(im); free(jm); free(isbeta); free(dist); free(xcoord); free(ycoord);
        return -1;
    }
    for (int j = 0; j < ny; j++)
        for (int k = 1; k <= 8; k++) dist[(size_t)j * 9 + k] = (float)sqrt(dxc[j] * dxc[j] * DX_[k] * DX_[k] + dyc[j] * dyc[j] * DY_[k] * DY_[k]);
    double dlon = 1., dlat = 1.;
    if (!path) {
        dlon = geo[2]; dlat = geo[3];
        const double xllcenter = geo[0] + dlon / 2., yllcenter = geo[1] - (ny * dlat) - dlat / 2.;
        const double b0 = xllcenter - (dlon / 2), b1 = yllcenter - (dlat / 2), b3 = b1 + (dlat * ny);
        for (int j = 0; j < ny; j++) ycoord[j] = (float)(b3 - (j * dlat));
        for (int i = 0; i < nx; i++) xcoord[i] = (float)(b0 + (i * dlon));
    }
    const double boa = ELIPB_ / ELIPA_;
    size_t head = 0, tail = 0;
    for (size_t c = 0; c < n; c++) { rz[c] = -FLT_MAX; dfs[c] = -FLT_MAX; zm[c] = -FLT_MAX; im[c] = -1; jm[c] = -1; if (taint) taint[c] = 0; }
    init_queue(nx, ny, ang, ang_nd, dxc, dyc, waiting, queue, &tail);
    while (head < tail) {
        const size_t c = queue[head++];
        const int i = (int)(c % (size_t)nx), j = (int)(c / (size_t)nx);
        if (!nodata_f(fel[c], fel_nd)) {
            if (ass[c] != ass_nd && ass[c] > 0) { rz[c] = alpha; im[c] = i; jm[c] = j; zm[c] = fel[c]; dfs[c] = 0.0f; }
            float rzzij = rz[c];
            int bad = 0;
            for (int k = 1; k <= 8; k++) {
                const int in = i + DX_[k], jn = j + DY_[k];
                if (in < 0 || in >= nx || jn < 0 || jn >= ny) continue;
                const size_t cn = (size_t)jn * nx + in;
                if (nodata_f(ang[cn], ang_nd)) continue;
                const double p = prop_(ang[cn], (k + 4) % 8, dxc[jn], dyc[jn]);
                if (!(p > 0.0 && p >= thresh)) continue;
                if (taint && taint[cn]) bad = 1;
                const float rzz = rz[cn];
                if (isbeta[cn] && ulps_(rzz, alpha) <= tol) bad = 1;   /* rz_contributor >= alpha could flip */
                if (!(rzz >= alpha)) continue;
                float d;
                if (path) d = dfs[cn] + dist[(size_t)j * 9 + k];
                else {
                    const float dxx = xcoord[i] - xcoord[im[cn]], dyy = ycoord[j] - ycoord[jm[cn]];
                    if (geographic) {   /* tiffIO::geotoLength(dxx, dyy, ycoord[j], .), src/tiffIO.cpp:434-445 */
                        double gdlat = dyy, gdlon = dxx, lat = ycoord[j];
                        gdlat = gdlat * PI_ / 180.; gdlon = gdlon * PI_ / 180.; lat = lat * PI_ / 180.;
                        const double beta = atan(boa * tan(lat));
                        const double dbeta = gdlat * boa * (cos(beta) / cos(lat)) * (cos(beta) / cos(lat));
                        const double ds2 = (pow(ELIPA_ * sin(beta), 2) + pow(ELIPB_ * cos(beta), 2)) * pow(dbeta, 2);
                        const double xc = ELIPA_ * cos(beta) * fabs(gdlon), yc = sqrt(ds2);
                        d = (float)sqrt(xc * xc + yc * yc);
                    } else d = sqrtf(dxx * dxx + dyy * dyy);
                }
                const float zd = zm[cn] - fel[c];
                const float beta = (float)(atanf(zd / d) * 180 / PI_);
                const int same = rzzij != -FLT_MAX && zm[cn] == zm[c] && d == dfs[c] && im[cn] == im[c] && jm[cn] == jm[c];   /* the record would not change */
                if (!same) {
                    const int wins_rz = beta > rzzij || ulps_(beta, rzzij) <= (isbeta[c] ? 2 * tol : tol);
                    if (ulps_(beta, alpha) <= tol && wins_rz) bad = 1;                                         /* beta >= alpha could flip */
                    if (rzzij != -FLT_MAX && ulps_(beta, rzzij) <= (isbeta[c] ? 2 * tol : tol) && (beta >= alpha || ulps_(beta, alpha) <= tol)) bad = 1;   /* beta > rz so far could flip */
                }
                if (beta >= alpha && beta > rzzij) {
                    rzzij = beta;
                    rz[c] = rzzij; im[c] = im[cn]; jm[c] = jm[cn]; zm[c] = zm[cn]; dfs[c] = d;
                    isbeta[c] = 1;
                }
            }
            if (taint && bad) taint[c] = 1;
        }
        release(nx, ny, ang, dxc, dyc, i, j, waiting, queue, &tail);
    }
    free(waiting); free(queue); free(zm); free(im); free(jm); free(isbeta); free(dist); free(xcoord); free(ycoord);
    return 0;
}
