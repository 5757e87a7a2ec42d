// Stand-alone check of SinmapSI's host side (taudem_amd/csrc/sinmap_table.cpp, the file the library is built from): reads the -calpar files named on the
// command line and prints, per file, the return code, the error text and the table with every float as its bit pattern, then the derived device table
// (tan of the friction angles and r as bit patterns) and the id lookup of a few cal values.  Built by tests/test_sinmap_calpar.py; it is also the
// program to build with -fsanitize=address,undefined.
#include <cstdio>
#include <cstring>
#include <string>

#include "sinmap_table.hpp"

static unsigned bits(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
static unsigned long long bits(double d) { unsigned long long u; memcpy(&u, &d, 8); return u; }

int main(int argc, char** argv) {
    for (int a = 1; a < argc; a++) {
        sinmap::Regions r;
        std::string err;
        const int rc = sinmap::read_calpar(argv[a], r, err);
        printf("file %d rc %d regions %zu err %s\n", a, rc, r.size(), rc ? err.c_str() : "-");
        for (size_t k = 0; k < r.size(); k++)
            printf("  %d %08x %08x %08x %08x %08x %08x %08x\n", r.id[k], bits(r.tmin[k]), bits(r.tmax[k]), bits(r.cmin[k]), bits(r.cmax[k]), bits(r.phimin[k]), bits(r.phimax[k]),
                   bits(r.rhos[k]));
        if (rc != 0) continue;
        std::vector<double> table;
        std::vector<int16_t> lut;
        sinmap::derive(int32_t(r.size()), r.id.data(), r.tmin.data(), r.tmax.data(), r.cmin.data(), r.cmax.data(), r.phimin.data(), r.phimax.data(), r.rhos.data(), 1000.0f,
                       -32768.0, table, lut);
        for (size_t k = 0; k < r.size(); k++)
            printf("  derived %zu %016llx %016llx %016llx\n", k, bits(table[k * sinmap::REG_STRIDE + 4]), bits(table[k * sinmap::REG_STRIDE + 5]), bits(table[k * sinmap::REG_STRIDE + 6]));
        const int probe[] = {-32768, -3, 0, 1, 2, 7, 8, 99, 300, 32767};
        printf("  lut");
        for (int v : probe) printf(" %d:%d", v, int(lut[uint16_t(int16_t(v))]));
        printf("\n");
    }
    return 0;
}
