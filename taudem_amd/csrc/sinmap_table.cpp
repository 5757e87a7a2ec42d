// SinmapSI's host side (sinmap_table.hpp).
#include "sinmap_table.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>

namespace sinmap {

int read_calpar(const char* path, Regions& r, std::string& err) {
    r = Regions();
    FILE* fp = fopen(path, "r");
    if (!fp) { err = std::string("cannot open ") + path; return 15; }
    char line[4096];
    int lineno = 0;
    while (fgets(line, sizeof line, fp)) {
        lineno++;
        if (lineno == 1) continue;   // the header text
        if (strspn(line, " \t\r\n\f\v") == strlen(line)) continue;   // the reference repeats its last region for such a line: the same table under first match
        int id;
        float v[7];
        const int got = sscanf(line, "%i,%f,%f,%f,%f,%f,%f,%f \n", &id, &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6]);
        if (got != 8) {
            fclose(fp);
            err = std::string(path) + ": line " + std::to_string(lineno) + " has " + std::to_string(got < 0 ? 0 : got) + " of the 8 fields id,tmin,tmax,cmin,cmax,phimin,phimax,rhos";
            return -1;
        }
        r.id.push_back(id);
        r.tmin.push_back(v[0]); r.tmax.push_back(v[1]); r.cmin.push_back(v[2]); r.cmax.push_back(v[3]);
        r.phimin.push_back(v[4]); r.phimax.push_back(v[5]); r.rhos.push_back(v[6]);
    }
    fclose(fp);
    return 0;
}

void derive(int32_t nreg, const int32_t* id, const float* tmin, const float* tmax, const float* cmin, const float* cmax, const float* phimin, const float* phimax,
            const float* rhos, float rhow, double cal_nodata, std::vector<double>& table, std::vector<int16_t>& lut) {
    const double PI = 3.14159265358979;   // as the reference writes it, not M_PI
    table.assign(size_t(nreg) * REG_STRIDE, 0.0);
    lut.assign(LUT_SIZE, int16_t(-1));
    for (int32_t k = nreg - 1; k >= 0; k--) {   // downwards: the first entry of an id is the one that stays
        const float t1 = float(phimin[k] * PI / 180), t2 = float(phimax[k] * PI / 180);   // stored as float, widened again when sindexcell is called
        const float r = rhow / rhos[k];
        double* e = &table[size_t(k) * REG_STRIDE];
        e[0] = tmin[k]; e[1] = tmax[k]; e[2] = cmin[k]; e[3] = cmax[k];
        e[4] = tan(double(t1)); e[5] = tan(double(t2));
        e[6] = r;
        if (id[k] >= -32768 && id[k] <= 32767) lut[uint16_t(int16_t(id[k]))] = int16_t(k);
    }
    // ndvter = (short)cal.getNodata(): a value outside the int range converts to INT_MIN on x86-64, whose low half is 0
    int32_t nd32 = (std::isfinite(cal_nodata) && cal_nodata > -2147483649.0 && cal_nodata < 2147483648.0) ? int32_t(cal_nodata) : INT32_MIN;
    lut[uint16_t(int16_t(nd32))] = int16_t(-1);
}

}  // namespace sinmap
