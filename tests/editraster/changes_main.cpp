// Stand-alone driver of taudem_amd/csrc/editraster_changes.cpp (no library, no HIP): what tests/test_editraster_host.py runs, and the program to build
// with -fsanitize=address,undefined when the reader or the selection changes.
//
//   changes_main read <change file>                       "status n" and one "x y value" line (%.17g) per record
//   changes_main select <nx> <row_lo> <row_hi> < list     the list: "col row value" lines; "refused", or one "cell value" line per kept change
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "editraster_changes.hpp"

int main(int argc, char** argv) {
    if (argc == 3 && strcmp(argv[1], "read") == 0) {
        std::vector<tdx::RasterChange> ch;
        const int rc = tdx::read_raster_changes(argv[2], ch);
        printf("%d %zu\n", rc, ch.size());
        for (const tdx::RasterChange& c : ch) printf("%.17g %.17g %d\n", c.x, c.y, c.val);
        return 0;
    }
    if (argc == 5 && strcmp(argv[1], "select") == 0) {
        std::vector<int32_t> cols, rows, vals;
        long c, r, v;
        while (scanf("%ld %ld %ld", &c, &r, &v) == 3) { cols.push_back(int32_t(c)); rows.push_back(int32_t(r)); vals.push_back(int32_t(v)); }
        std::vector<uint32_t> cell;
        std::vector<int16_t> val;
        if (!tdx::select_raster_changes(cols.data(), rows.data(), vals.data(), int64_t(cols.size()), atoll(argv[2]), atoll(argv[3]), atoll(argv[4]), cell, val)) {
            printf("refused\n");
            return 0;
        }
        for (size_t i = 0; i < cell.size(); i++) printf("%u %d\n", cell[i], int(val[i]));
        return 0;
    }
    fprintf(stderr, "usage: changes_main read <file> | select <nx> <row_lo> <row_hi>\n");
    return 2;
}
