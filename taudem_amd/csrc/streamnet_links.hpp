// StreamNet's link builder (src/streamnet.cpp:668-959 with the link set of src/linklib.h) over the COMPACT stream cells: the irregular tenth of
// the tool, a FIFO walk over the stream cells alone, on the host.  Plain C++, no HIP headers (streamnet.hip makes the compact arrays on the device).
#pragma once
#include <cstdint>
#include <vector>

namespace streamnet {

constexpr int32_t LINK_NONE = -2147483647;   // MISSINGLONG (src/commonLib.h:79): idGrid's / wsGrid's nodata, "no outlet on this cell"
constexpr uint8_t CELL_TERMINAL = 1;         // the receiver is off the raster, or its src is nodata or != 1 (src/streamnet.cpp:764-766)

// The stream cells (src not nodata, src > 0, p not nodata: src/streamnet.cpp:567) in row-major order.
struct Compact {
    int64_t n = 0;
    const int64_t* idx = nullptr;      // linear index in the raster
    const int16_t* p = nullptr;        // direction code
    const float* fel = nullptr;
    const float* ad8 = nullptr;
    const float* len = nullptr;        // distance to the outlet along the stream, MISSINGFLOAT above a cycle
    const int32_t* outlet = nullptr;   // id of the (last) outlet on the cell, or LINK_NONE
    const int32_t* recv = nullptr;     // compact rank of the receiver where that is a stream cell, else -1
    const uint8_t* flags = nullptr;    // CELL_TERMINAL
};

struct Links {
    std::vector<int64_t> tree;     // 9 per link, the -tree file's columns in its order of rows (src/linklib.h:800-846)
    std::vector<double> coord;     // 5 per point, the -coord file's columns; a link's points are rows tree[1] .. tree[2]
    std::vector<int32_t> label;    // per stream cell: wsGrid, LINK_NONE where the walk never came (on or below a cycle)
    std::vector<int16_t> order;    // per stream cell: the Strahler order, 0 where the walk never came
};

// gt: {x of the left edge, cell width, y of the top edge, cell height}; dxA * dyA is the cell area of the -coord file's last column.
void build_links(const Compact& C, int64_t nx, double dxA, double dyA, const double* gt, Links& out);

}  // namespace streamnet
