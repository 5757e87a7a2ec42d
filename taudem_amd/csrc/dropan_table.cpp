// Host side of DropAnalysis: see dropan_table.hpp.  Plain C++ (the Makefile compiles this file without -x hip).
#include "dropan_table.hpp"

#include <math.h>
#include <stdio.h>

#include <iomanip>
#include <iostream>
#include <sstream>

using namespace std;   // as in the reference: sqrt / log / exp of a float are the float overloads, pow(float, int) goes through double

namespace dropan {

float ladder(float threshmin, float threshmax, int nthresh, int steptype, int th) {
    float thresh;
    if (steptype == 0) {   // src/DropAnalysis.cpp:380-381
        float r = exp((log(threshmax) - log(threshmin)) / (nthresh - 1));
        thresh = threshmin * pow(r, th);
    } else {               // src/DropAnalysis.cpp:383-384
        float delta = (threshmax - threshmin) / (nthresh - 1);
        thresh = threshmin + th * delta;
    }
    return thresh;
}

void table(const Sums& s, std::string* table, std::string* console, float* optimum, int* found) {
    ostringstream con;
    string tab = "Threshold, DrainDen, NoFirstOrd,NoHighOrd, MeanDFirstOrd, MeanDHighOrd, StdDevFirstOrd, StdDevHighOrd, T\n";
    con << "Threshold DrainDen NoFirstOrd NoHighOrd MeanDFirstOrd MeanDHighOrd StdDevFirstOrd StdDevHighOrd Tval" << endl;
    bool optnotset = true;
    float threshopt = 0.f;   // (the reference leaves it uninitialised when no threshold qualifies)
    char line[512];
    for (int64_t th = 0; th < s.nthresh; th++) {
        const float thresh = s.thresh[th];
        const float gs1 = s.s1[th], gs2 = s.s2[th], gs1sq = s.s1sq[th], gs2sq = s.s2sq[th];
        const double glen = s.length[th];
        const int gn1 = int(s.n1[th]), gn2 = int(s.n2[th]);
        const float totalAreaProcessed = s.total_area;
        // src/DropAnalysis.cpp:597-637, expression by expression
        float drainden = glen / totalAreaProcessed;
        con << setiosflags(ios::fixed) << setprecision(6) << thresh << " " << drainden << " " << gn1 << " " << gn2 << " ";
        float md1 = gs1 / gn1;
        if (gn1 > 0) con << md1; else con << " - ";
        con << " ";
        float mdh = gs2 / gn2;
        if (gn2 > 0) con << mdh; else con << " - ";
        con << " ";
        float sd1 = sqrt((gs1sq - gn1 * md1 * md1) / (gn1 - 1));
        if (gn1 > 1) con << sd1; else con << " - ";
        con << " ";
        float sdh = sqrt((gs2sq - gn2 * mdh * mdh) / (gn2 - 1));
        if (gn2 > 1) con << sdh; else con << " - ";
        con << " ";
        float t = (md1 - mdh) / (sqrt(((gn1 - 1) * sd1 * sd1 + (gn2 - 1) * sdh * sdh) / (gn1 + gn2 - 2)) * sqrt(1. / gn1 + 1. / gn2));
        if (gn2 > 1) con << t; else con << " - ";
        con << endl;
        if (fabs(t) < 2. && optnotset) {   // the first one is the optimum; a NaN t never qualifies
            threshopt = thresh;
            optnotset = false;
        }
        if (gn1 > 1 && gn2 > 1) {
            snprintf(line, sizeof line, "%f, %e, %d, %d, %f, %f, %f, %f, %f\n", thresh, drainden, gn1, gn2, md1, mdh, sd1, sdh, t);
            tab += line;
        }
    }
    snprintf(line, sizeof line, "%f  Value for optimum that drop analysis selected - see output file for details.\n", threshopt);
    con << line;
    snprintf(line, sizeof line, "Optimum Threshold Value: %f\n", threshopt);
    tab += line;
    if (table) *table = tab;
    if (console) *console = con.str();
    if (optimum) *optimum = threshopt;
    if (found) *found = optnotset ? 0 : 1;
}

}  // namespace dropan
