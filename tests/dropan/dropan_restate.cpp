// A serial C++ restatement of DropAnalysis (dropan, src/DropAnalysis.cpp) on one rank, written from the rules of DESIGN.md section "DropAnalysis": a FIFO
// queue filled in row-major order, float sums added in the order the queue pops the cells - the order-dependent part of the reference, which the GPU code
// does not share and this file is there to pin.  Its CPU test holds its table to every 1-rank golden byte for byte.  It also hands out what the table
// does not show: the drop lists in pop order, the order grid and the elevOut grid of one threshold.  Built by the tests with
// `g++ -O2 -ffp-contract=off -shared -fPIC`; <math.h> and `using namespace std` give the expressions the overloads they have in the reference.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <iomanip>
#include <iostream>
#include <queue>
#include <sstream>
#include <string>
#include <vector>
using namespace std;

static const int D1[9] = {0, 1, 1, 0, -1, -1, -1, 0, 1};
static const int D2[9] = {0, 0, -1, -1, -1, 0, 1, 1, 1};
static const int16_t NO_ORDER = -32768;
static const float NO_ELEV = -3.402823466e38f;

static bool nodata_f(float v, float nd) { return fabsf((float)(v - nd)) < 1e-5f; }

struct Grid {
    int nx, ny;
    const int16_t* p; int16_t p_nd;
    const float* ssa; float ssa_nd;
    bool inside(int x, int y) const { return x >= 0 && x < nx && y >= 0 && y < ny; }
    bool on_mask(int x, int y, float thresh) const { const float v = ssa[(size_t)y * nx + x]; return !nodata_f(v, ssa_nd) && v >= thresh; }
    // neighbour (xn, yn) has a direction that points at (x, y)
    bool points_to(int x, int y, int xn, int yn) const {
        if (!inside(xn, yn)) return false;
        const int16_t d = p[(size_t)yn * nx + xn];
        if (d == p_nd || d < 1 || d > 8) return false;
        return yn + D2[d] == y && xn + D1[d] == x;
    }
};

extern "C" {

// the threshold ladder, in float
void da_ladder(float threshmin, float threshmax, int nthresh, int steptype, float* out) {
    for (int th = 0; th < nthresh; ++th) {
        float thresh;
        if (steptype == 0) {
            float r = exp((log(threshmax) - log(threshmin)) / (nthresh - 1));
            thresh = threshmin * pow(r, th);
        } else {
            float delta = (threshmax - threshmin) / (nthresh - 1);
            thresh = threshmin + th * delta;
        }
        out[th] = thresh;
    }
}

// One threshold.  s: s1, s1sq, s2, s2sq in float, queue order; n: n1, n2; length: double, queue order.  order / elev (may be null): the grids; drops1 / drops2
// (may be null, room for nx * ny each): the first-order and the higher-order drops in the order they were added.
void da_threshold(int nx, int ny, const int16_t* p, int16_t p_nd, const float* fel, const float* ssa, float ssa_nd, const double* dxc, const double* dyc, float thresh,
                  float* s, int64_t* n, double* length_out, int16_t* order_out, float* elev_out, float* drops1, float* drops2) {
    const Grid g{nx, ny, p, p_nd, ssa, ssa_nd};
    const size_t cells = (size_t)nx * ny;
    vector<int> contribs(cells, -1);           // -1: not on the mask
    vector<int16_t> order(cells, NO_ORDER);
    vector<float> elev(cells, NO_ELEV);
    float s1 = 0.0, s2 = 0.0, s1sq = 0.0, s2sq = 0.0;
    long n1 = 0, n2 = 0;
    double length = 0.0;
    for (int j = 0; j < ny; ++j)
        for (int i = 0; i < nx; ++i) {
            int k = 0;
            for (int m = 1; m <= 8; ++m) {
                const int xn = i + D1[m], yn = j + D2[m];
                if (g.points_to(i, j, xn, yn) && g.on_mask(xn, yn, thresh)) k++;
            }
            if (g.on_mask(i, j, thresh)) contribs[(size_t)j * nx + i] = k;
        }
    queue<pair<int, int>> que;
    for (int j = 0; j < ny; ++j)
        for (int i = 0; i < nx; ++i)
            if (contribs[(size_t)j * nx + i] == 0) que.push({i, j});
    while (!que.empty()) {
        const int i = que.front().first, j = que.front().second;
        que.pop();
        const size_t c = (size_t)j * nx + i;
        short nOrder[8];
        int pi = 0, pj = 0;
        for (int k = 0; k < 8; ++k) nOrder[k] = 0;
        for (int m = 1; m <= 8; ++m) {
            const int xn = i + D1[m], yn = j + D2[m];
            if (g.points_to(i, j, xn, yn) && order[(size_t)yn * nx + xn] != NO_ORDER) {
                nOrder[m - 1] = order[(size_t)yn * nx + xn];
                pi = xn; pj = yn;
                const double tempdxc = dxc[j], tempdyc = dyc[j];
                if (m == 1 || m == 5) length = length + tempdxc;
                if (m == 3 || m == 7) length = length + tempdyc;
                if (m % 2 == 0) length = length + sqrt(tempdxc * tempdxc + tempdyc * tempdyc);
            }
        }
        // the order rule: a scan in neighbour order
        short oOut = 1, ordermax = 0, count = 0;
        bool junction = false, source = true;
        for (int k = 0; k < 8; k++)
            if (nOrder[k] > 0) {
                count = count + 1;
                source = false;
                if (count == 1) { oOut = nOrder[k]; ordermax = nOrder[k]; }
                else {
                    if (nOrder[k] > oOut) { ordermax = nOrder[k]; oOut = nOrder[k]; }
                    else if (nOrder[k] == oOut) oOut = ordermax + 1;
                    junction = true;
                }
            }
        order[c] = oOut;
        if (source) elev[c] = fel[c];
        else if (!junction) elev[c] = elev[(size_t)pj * nx + pi];
        else {
            bool newstream = true;
            for (int k = 1; k <= 8; ++k) {
                const int xn = i + D1[k], yn = j + D2[k];
                if (!g.points_to(i, j, xn, yn) || order[(size_t)yn * nx + xn] == NO_ORDER) continue;
                const short o = order[(size_t)yn * nx + xn];
                if (o < oOut) {
                    float drop = elev[(size_t)yn * nx + xn] - fel[c];
                    if (o == 1) {
                        s1 = s1 + drop;
                        s1sq = s1sq + drop * drop;
                        if (drops1) drops1[n1] = drop;
                        n1 = n1 + 1;
                    } else {
                        s2 = s2 + drop;
                        s2sq = s2sq + drop * drop;
                        if (drops2) drops2[n2] = drop;
                        n2 = n2 + 1;
                    }
                } else {
                    elev[c] = elev[(size_t)yn * nx + xn];
                    newstream = false;
                }
            }
            if (newstream) elev[c] = fel[c];
        }
        const int16_t d = p[c];
        if (d != p_nd && d >= 1 && d <= 8) {
            const int xn = i + D1[d], yn = j + D2[d];
            if (g.inside(xn, yn) && contribs[(size_t)yn * nx + xn] > 0) {
                if (--contribs[(size_t)yn * nx + xn] == 0) que.push({xn, yn});
            }
        }
    }
    s[0] = s1; s[1] = s1sq; s[2] = s2; s[3] = s2sq;
    n[0] = n1; n[1] = n2;
    *length_out = length;
    if (order_out) memcpy(order_out, order.data(), cells * sizeof(int16_t));
    if (elev_out) memcpy(elev_out, elev.data(), cells * sizeof(float));
}

// total area: returns -1 when an outlet inside the raster lies on a cell without a direction 0..8, else 0
int da_total_area(int nx, int ny, const float* ad8, const int16_t* p, int16_t p_nd, const float* ssa, float ssa_nd, const int32_t* ox, const int32_t* oy, int nout,
                  double dxA, double dyA, float* total) {
    const Grid g{nx, ny, p, p_nd, ssa, ssa_nd};
    float totalAreaProcessed = 0;
    for (int i = 0; i < nout; i++) {
        const int tx = ox[i], ty = oy[i];
        if (!g.inside(tx, ty)) continue;
        const float ta = ad8[(size_t)ty * nx + tx];
        const int16_t nd = p[(size_t)ty * nx + tx];
        if (nd == p_nd || nd < 0 || nd > 8) return -1;
        const int xn = tx + D1[nd], yn = ty + D2[nd];
        if (!g.inside(xn, yn) || nodata_f(ssa[(size_t)yn * nx + xn], ssa_nd) || ssa[(size_t)yn * nx + xn] <= 0) totalAreaProcessed += ta;
    }
    const float ta = totalAreaProcessed;
    totalAreaProcessed = ta * dxA * dyA;
    *total = totalAreaProcessed;
    return 0;
}

// the table file and the console lines from the float sums; returns the bytes of the table (without the NUL), -1 when a buffer is too small
int da_table(int nthresh, const float* thresh, const int64_t* n1, const int64_t* n2, const float* s1, const float* s1sq, const float* s2, const float* s2sq,
             const double* length, float totalAreaProcessed, char* table, int table_cap, char* console, int console_cap, float* threshopt, int* found) {
    string tab = "Threshold, DrainDen, NoFirstOrd,NoHighOrd, MeanDFirstOrd, MeanDHighOrd, StdDevFirstOrd, StdDevHighOrd, T\n";
    ostringstream cout_;
    cout_ << "Threshold" << " DrainDen" << " NoFirstOrd" << " NoHighOrd" << " MeanDFirstOrd" << " MeanDHighOrd" << " StdDevFirstOrd" << " StdDevHighOrd" << " Tval" << endl;
    bool optnotset = true;
    *threshopt = 0.f;
    char buf[512];
    for (int th = 0; th < nthresh; ++th) {
        const float gs1 = s1[th], gs2 = s2[th], gs1sq = s1sq[th], gs2sq = s2sq[th];
        const double glen = length[th];
        const int gn1 = (int)n1[th], gn2 = (int)n2[th];
        float drainden = glen / totalAreaProcessed;
        cout_ << setiosflags(ios::fixed) << setprecision(6) << thresh[th];
        cout_ << " " << drainden << " " << gn1 << " " << gn2 << " ";
        float md1 = gs1 / gn1;
        if (gn1 > 0) cout_ << md1; else cout_ << " - ";
        cout_ << " ";
        float mdh = gs2 / gn2;
        if (gn2 > 0) cout_ << mdh; else cout_ << " - ";
        cout_ << " ";
        float sd1 = sqrt((gs1sq - gn1 * md1 * md1) / (gn1 - 1));
        if (gn1 > 1) cout_ << sd1; else cout_ << " - ";
        cout_ << " ";
        float sdh = sqrt((gs2sq - gn2 * mdh * mdh) / (gn2 - 1));
        if (gn2 > 1) cout_ << sdh; else cout_ << " - ";
        cout_ << " ";
        float t = (md1 - mdh) / (sqrt(((gn1 - 1) * sd1 * sd1 + (gn2 - 1) * sdh * sdh) / (gn1 + gn2 - 2)) * sqrt(1. / gn1 + 1. / gn2));
        if (gn2 > 1) cout_ << t; else cout_ << " - ";
        cout_ << endl;
        if (fabs(t) < 2. && optnotset) { *threshopt = thresh[th]; optnotset = false; }
        if (gn1 > 1 && gn2 > 1) {
            snprintf(buf, sizeof buf, "%f, %e, %d, %d, %f, %f, %f, %f, %f\n", thresh[th], drainden, gn1, gn2, md1, mdh, sd1, sdh, t);
            tab += buf;
        }
    }
    snprintf(buf, sizeof buf, "%f  Value for optimum that drop analysis selected - see output file for details.\n", *threshopt);
    cout_ << buf;
    snprintf(buf, sizeof buf, "Optimum Threshold Value: %f\n", *threshopt);
    tab += buf;
    *found = optnotset ? 0 : 1;
    const string con = cout_.str();
    if ((int)tab.size() + 1 > table_cap || (console && (int)con.size() + 1 > console_cap)) return -1;
    memcpy(table, tab.c_str(), tab.size() + 1);
    if (console) memcpy(console, con.c_str(), con.size() + 1);
    return (int)tab.size();
}

}  // extern "C"
