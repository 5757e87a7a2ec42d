// SinmapSI's cell loop on one rank, restated from the tool's description: region lookup, nodata rules, the wetness bounds, the stability index with its five
// outcomes and the probability integrals behind regions 1 to 3.  REAL is the type of all cell arithmetic: double (built with -ffp-contract=off this is the
// reference's arithmetic; built with -ffp-contract=fast -march=native it is what a contracting compiler may make of it) or long double.  The inputs keep
// the reference's value types whatever REAL is: float rasters, float region fields, float(phi * PI / 180), the float division rhow / rhos, double recharge.
// Every cell also gets a path code (tests/sinmap_model.py names them).
#include <algorithm>
#include <cmath>
#include <cstdint>

#ifndef REAL
#define REAL double
#endif
typedef REAL real;

namespace {

enum { NODATA = 0, NOT_WRITTEN = 1, FLAT = 2, UNSTABLE = 3, STABLE = 4, REGION1 = 5, REGION2 = 10, REGION3 = 20 };
enum { F3_ORDER = 0, F3_NEGATIVE = 1, F3_DEGENERATE = 2, F3_FA = 3, F3_FAI = 4 };

// P(u + v <= z) for u uniform on [ulo, uhi] and v uniform on [vlo, vhi].  The density of the sum is a trapezoid: it rises over the shorter of the two
// ranges, is level up to the second knee and falls to the top.  The tool tests the four pieces from the bottom up and lets a later one overwrite an
// earlier one; here they are asked from the top down and the first that holds is taken, which is the same choice (none holds for a NaN: 0).
real f2s(real ulo, real uhi, real vlo, real vhi, real z) {
    const real corner_a = ulo + vhi, corner_b = uhi + vlo, bottom = ulo + vlo, top = uhi + vhi;
    const real knee1 = std::min(corner_a, corner_b), knee2 = std::max(corner_a, corner_b);
    const real du = uhi - ulo, dv = vhi - vlo;
    const real shorter = std::min(du, dv), longer = std::max(du, dv);
    const real up = z - vlo - ulo;
    if (z >= top) return 1;
    if (knee2 < z && z < top) {
        const real down = z - vhi - uhi;
        return 1 - down * down / (2 * du * dv);
    }
    if (knee1 <= z && z <= knee2) return (up - shorter / 2) / longer;
    if (z > bottom && z < knee1) return up * up / (2 * du * dv);
    return 0;
}

// The antiderivatives of the product distribution's pieces (y in [y1, y2] times b in [b1, b2], argument a), each over the rectangle's area
real area(real y1, real y2, real b1, real b2) { return (y2 - y1) * (b2 - b1); }
real fai2(real y1, real y2, real b1, real b2, real a) { return (a * a * std::log(a / (y1 * b1)) / 2 - 3 * a * a / 4 + y1 * b1 * a) / area(y1, y2, b1, b2); }
real fai3(real y1, real y2, real b1, real b2, real a) { return (a * a * std::log(b2 / b1) / 2 - (b2 - b1) * y1 * a) / area(y1, y2, b1, b2); }
real fai4(real y1, real y2, real b1, real b2, real a) {
    return (a * a * std::log(b2 * y2 / a) / 2 + 3 * a * a / 4 + b1 * y1 * a - b1 * y2 * a - b2 * y1 * a) / area(y1, y2, b1, b2);
}
real fai5(real, real, real, real, real a) { return a; }

// Both integrals want the pair with the smaller cross product first: y and b trade places when y1 * b2 > y2 * b1
struct Pairs { real y1, y2, b1, b2; };
Pairs ordered(real y1, real y2, real b1, real b2) {
    if (y1 * b2 > y2 * b1) return Pairs{b1, b2, y1, y2};
    return Pairs{y1, y2, b1, b2};
}

// The integral of the product's distribution up to a: four pieces between the corner products, joined by the constants k2..k5 so that it is continuous.
// Asked from the top piece down, as in f2s.
real fai(real y1_in, real y2_in, real b1_in, real b2_in, real a) {
    const Pairs q = ordered(y1_in, y2_in, b1_in, b2_in);
    const real y1 = q.y1, y2 = q.y2, b1 = q.b1, b2 = q.b2;
    const real lo = y1 * b1, mid1 = y1 * b2, mid2 = y2 * b1, hi = y2 * b2;
    const real k2 = -fai2(y1, y2, b1, b2, lo);
    real k3 = 0, k4 = 0;
    if (!(mid1 == 0)) k3 = fai2(y1, y2, b1, b2, mid1) + k2 - fai3(y1, y2, b1, b2, mid1);
    if (!(mid2 == 0)) k4 = fai3(y1, y2, b1, b2, mid2) + k3 - fai4(y1, y2, b1, b2, mid2);
    const real k5 = fai4(y1, y2, b1, b2, hi) + k4 - fai5(y1, y2, b1, b2, hi);
    if (a >= hi) return fai5(y1, y2, b1, b2, a) + k5;
    if (mid2 < a && a < hi) return fai4(y1, y2, b1, b2, a) + k4;
    if (mid1 < a && a <= mid2) return fai3(y1, y2, b1, b2, a) + k3;
    if (lo < a && a <= mid1) return fai2(y1, y2, b1, b2, a) + k2;
    return 0;
}

// The product's distribution itself at a (used when the additive term has no width)
real fa(real y1_in, real y2_in, real b1_in, real b2_in, real a) {
    const Pairs q = ordered(y1_in, y2_in, b1_in, b2_in);
    const real y1 = q.y1, y2 = q.y2, b1 = q.b1, b2 = q.b2;
    const real whole = area(y1, y2, b1, b2);
    if (a >= b2 * y2) return 1;
    if (y2 * b1 < a && a < y2 * b2) return (a * std::log((b2 * y2) / a) + a + b1 * y1 - b1 * y2 - b2 * y1) / whole;
    if (y1 * b2 < a && a <= y2 * b1) return (a * std::log(b2 / b1) - (b2 - b1) * y1) / whole;
    if (y1 * b1 < a && a <= y1 * b2) return (a * std::log(a / (y1 * b1)) - a + y1 * b1) / whole;
    return 0;
}

real f3s(real x1, real x2, real y1, real y2, real b1, real b2, real z, int& sub) {
    if (x2 < x1 || y2 < y1 || b2 < b1) { sub = F3_ORDER; return 1000; }
    if (x1 < 0 || y1 < 0 || b1 < 0) { sub = F3_NEGATIVE; return 1000; }
    if (y1 == y2 || b1 == b2) { sub = F3_DEGENERATE; return f2s(x1, x2, y1 * b1, y2 * b2, z); }
    if (x2 == x1) { sub = F3_FA; return fa(y1, y2, b1, b2, z - x1); }
    sub = F3_FAI;
    return (fai(y1, y2, b1, b2, z - x1) - fai(y1, y2, b1, b2, z - x2)) / (x2 - x1);
}

real fs(real s, real w, real c, real t, real r) {
    const real cs = std::cos(s), ss = std::sin(s);
    return (c + cs * (1 - w * r) * t) / ss;
}

real sindexcell(real s, real a, real c1, real c2, real t1, real t2, real x1, real x2, real r, real* sat, int* code) {
    if (s == 0) { *sat = 3; *code = FLAT; return 10; }
    s = std::atan(s);
    t1 = std::tan(t1);
    t2 = std::tan(t2);
    const real cs = std::cos(s), ss = std::sin(s);
    if (x1 > x2) std::swap(x1, x2);
    real w2 = x2 * a / ss, w1 = x1 * a / ss;
    *sat = w2;
    if (w2 > 1) { w2 = 1; *sat = 2; }
    if (w1 > 1) { w1 = 1; *sat = 3; }
    real si;
    int sub = 0;
    const real fs2 = fs(s, w1, c2, t2, r);
    if (fs2 < 1) { si = 0; *code = UNSTABLE; }
    else {
        const real fs1 = fs(s, w2, c1, t1, r);
        if (fs1 >= 1) { si = fs1; *code = STABLE; }
        else if (w1 == 1) {
            si = 1 - f2s(c1 / ss, c2 / ss, cs * (1 - r) / ss * t1, cs * (1 - r) / ss * t2, 1);
            *code = REGION1;
        } else if (w2 == 1) {
            const real as = a / ss, y1 = cs / ss * (1 - r), y2 = cs / ss * (1 - x1 * as * r);
            const real cdf1 = (x2 * as - 1) / (x2 * as - x1 * as) * f2s(c1 / ss, c2 / ss, cs * (1 - r) / ss * t1, cs * (1 - r) / ss * t2, 1);
            const real cdf2 = (1 - x1 * as) / (x2 * as - x1 * as) * f3s(c1 / ss, c2 / ss, y1, y2, t1, t2, 1, sub);
            si = 1 - cdf1 - cdf2;
            *code = REGION2 + sub;
        } else {
            const real as = a / ss, y1 = cs / ss * (1 - x2 * as * r), y2 = cs / ss * (1 - x1 * as * r);
            si = 1 - f3s(c1 / ss, c2 / ss, y1, y2, t1, t2, 1, sub);
            *code = REGION3 + sub;
        }
    }
    if (si > 10) si = 10;
    return si;
}

}  // namespace

// n cells; scamin / scamax may be null (0); the region table in file order; si and sat float32 with -1 where the tool writes nodata or nothing
extern "C" void sm_run(long n, const float* slp, const float* sca, const float* scamin, const float* scamax, const int16_t* cal, float slp_nodata, int cal_nodata_short,
                       int nreg, const int* id, const float* tmin, const float* tmax, const float* cmin, const float* cmax, const float* phimin, const float* phimax,
                       const float* rhos, double rminter, double rmaxter, float rhow, float* si, float* sat, uint8_t* code) {
    const double PI = 3.14159265358979;
    for (long i = 0; i < n; i++) {
        const float smin = scamin ? scamin[i] : 0.0f, smax = scamax ? scamax[i] : 0.0f;
        int k = -1;
        if (cal[i] != int16_t(cal_nodata_short))
            for (int j = 0; j < nreg; j++)
                if (int(cal[i]) == id[j]) { k = j; break; }
        si[i] = sat[i] = -1.0f;
        code[i] = NODATA;
        if (k < 0 || sca[i] < 0 || smin < 0 || smax < 0 || slp[i] == slp_nodata) continue;
        code[i] = NOT_WRITTEN;
        if (!(rmaxter != 0 || smax != 0)) continue;
        const float tphimin = float(phimin[k] * PI / 180), tphimax = float(phimax[k] * PI / 180), r = rhow / rhos[k];
        const real X2 = (real(sca[i]) * real(rmaxter) + real(smax)) / real(tmin[k]);
        const real X1 = (real(sca[i]) * real(rminter) + real(smin)) / real(tmax[k]);
        real cellsat = 0;
        int c = 0;
        si[i] = float(sindexcell(real(slp[i]), real(1), real(cmin[k]), real(cmax[k]), real(tphimin), real(tphimax), X1, X2, real(r), &cellsat, &c));
        sat[i] = float(cellsat);
        code[i] = uint8_t(c);
    }
}
