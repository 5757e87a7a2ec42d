// EditRaster's host side: the change file's reader (src/EditRaster.cpp:124-133) and the choice of the one change per cell that the device scatters.
// Plain C++ without HIP headers or a context: tests/editraster/changes_main.cpp builds the same file on its own.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace tdx {

struct RasterChange {
    double x, y;
    int32_t val;
};

enum { CHANGES_OK = 0, CHANGES_NO_FILE = 1, CHANGES_RANGE = 2 };
// The records of a change file in file order.  CHANGES_RANGE: the record after the ones returned holds a value no int16 holds.
int read_raster_changes(const std::string& path, std::vector<RasterChange>& out);

// Of changes k = 0 .. n - 1 (column, row, value) those in columns [0, nx) and rows [row_lo, row_hi), one per cell - the LAST in the list - in ascending
// cell order: cell = (row - row_lo) * nx + col.  false: a value of the list (on or off the raster) is outside -32768 .. 32767; nothing is returned then.
bool select_raster_changes(const int32_t* cols, const int32_t* rows, const int32_t* vals, int64_t n, int64_t nx, int64_t row_lo, int64_t row_hi,
                           std::vector<uint32_t>& cell, std::vector<int16_t>& val);

}  // namespace tdx
