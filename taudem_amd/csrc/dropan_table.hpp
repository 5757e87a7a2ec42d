// Host side of DropAnalysis (src/DropAnalysis.cpp:378-385, 597-674): the threshold ladder and the table, as plain C++ host code.
// dropan_table.cpp is compiled as C++, not as HIP, and writes the reference's expressions the way the reference does, so that the same
// float / double overloads of log, exp, pow and sqrt are picked.
#pragma once
#include <cstdint>
#include <string>

namespace dropan {

// threshold number th of the ladder (steptype 0: log steps, else arithmetic steps), in float
float ladder(float threshmin, float threshmax, int nthresh, int steptype, int th);

// What the sweeps of all thresholds leave: per threshold the threshold, the numbers of first-order and higher-order drops, their float sums and
// sums of squares and the stream length; and the total area.
struct Sums {
    int64_t nthresh;
    const float* thresh;
    const int64_t *n1, *n2;
    const float *s1, *s1sq, *s2, *s2sq;
    const double* length;
    float total_area;
};

// The table file (table), the console lines (console; either may be null) and the optimum: the first threshold with |t| < 2, found = 0 and
// optimum = 0 when there is none.
void table(const Sums& s, std::string* table, std::string* console, float* optimum, int* found);

}  // namespace dropan
