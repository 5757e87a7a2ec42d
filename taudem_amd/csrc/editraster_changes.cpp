#include "editraster_changes.hpp"

#include <algorithm>
#include <cstdio>

namespace tdx {

int read_raster_changes(const std::string& path, std::vector<RasterChange>& out) {
    out.clear();
    FILE* fp = fopen(path.c_str(), "r");
    if (!fp) return CHANGES_NO_FILE;
    // readline(fp, headers): up to MAXLN = 4096 characters, through the first newline (src/EditRaster.cpp:51-66)
    for (int i = 0; i < 4096; i++) {
        const int ch = getc(fp);
        if (ch == EOF || ch == '\n') break;
    }
    int rc = CHANGES_OK;
    double x, y;
    long v;   // the reference scans "%d" into a short; a long holds whatever the text says (strtol saturates), so that the range can be judged
    while (fscanf(fp, "%lf,%lf,%ld", &x, &y, &v) == 3) {
        if (v < -32768 || v > 32767) { rc = CHANGES_RANGE; break; }
        out.push_back({x, y, int32_t(v)});
    }
    fclose(fp);
    return rc;
}

bool select_raster_changes(const int32_t* cols, const int32_t* rows, const int32_t* vals, int64_t n, int64_t nx, int64_t row_lo, int64_t row_hi,
                           std::vector<uint32_t>& cell, std::vector<int16_t>& val) {
    cell.clear();
    val.clear();
    for (int64_t k = 0; k < n; k++)
        if (vals[k] < -32768 || vals[k] > 32767) return false;
    // (cell, position in the list) as one word: after the sort the last entry of a run of equal cells is the last change of that cell
    std::vector<std::pair<uint32_t, int64_t>> key;
    for (int64_t k = 0; k < n; k++) {
        const int64_t c = cols[k], r = rows[k];
        if (c < 0 || c >= nx || r < row_lo || r >= row_hi) continue;
        key.emplace_back(uint32_t((r - row_lo) * nx + c), k);
    }
    std::sort(key.begin(), key.end());
    for (size_t i = 0; i < key.size(); i++) {
        if (i + 1 < key.size() && key[i + 1].first == key[i].first) continue;
        cell.push_back(key[i].first);
        val.push_back(int16_t(vals[key[i].second]));
    }
    return true;
}

}  // namespace tdx
