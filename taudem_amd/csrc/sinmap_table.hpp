// SinmapSI's host side: the -calpar reader and what the reference derives per region before its cell loop (src/SinmapSI.cpp:183-221 and the first
// lines of sindexcell, :470-473).  Plain C++ without HIP headers, so that tan() and the float divisions are the host libm's and the host compiler's.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace sinmap {

struct Regions {
    std::vector<int32_t> id;
    std::vector<float> tmin, tmax, cmin, cmax, phimin, phimax, rhos;
    size_t size() const { return id.size(); }
};

// 0; 15: the file cannot be opened; -1: a data line with fewer than 8 fields (err names the line)
int read_calpar(const char* path, Regions& r, std::string& err);

constexpr int REG_STRIDE = 8;   // doubles per region in the device table: tmin tmax cmin cmax tan(phimin) tan(phimax) r 0
constexpr int LUT_SIZE = 65536;

// table: nreg * REG_STRIDE doubles.  lut: LUT_SIZE entries indexed by (uint16_t)cal, the index of the first region with that id, or -1; the entry
// of (int16_t)cal_nodata is -1.
void derive(int32_t nreg, const int32_t* id, const float* tmin, const float* tmax, const float* cmin, const float* cmax, const float* phimin, const float* phimax,
            const float* rhos, float rhow, double cal_nodata, std::vector<double>& table, std::vector<int16_t>& lut);

}  // namespace sinmap
