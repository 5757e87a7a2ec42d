// StreamNet's network layer from the link rows: reachshape() (src/streamnet.cpp:244-365) and the field list of createStreamNetShapefile() (:107-241).
// Plain C++ on the rows of the -tree and -coord files - no HIP headers, no context: tests/netlayer/netlayer_main.cpp builds the same file.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "vector_layer.hpp"

namespace streamnet {

constexpr int NET_REALS = 9;   // Length, DSContArea, strmDrop, Slope, StraightL, USContArea, DOUTEND, DOUTSTART, DOUTMID
struct NetRows {
    std::vector<double> real;     // NET_REALS per link, in tree order
    std::vector<int64_t> first;   // links + 1 offsets into x / y
    std::vector<double> x, y;     // the vertices of every link, REVERSED: vertex 0 is the link's downstream end
};

// tree [n_links][9], coord [n_points][5]: what tdx_streamnet_links_copy returns.  Columns 2..4 of coord hold float values and are used as floats.
// false: a link's coord rows lie outside coord (err says which).
bool net_rows(const int64_t* tree, const double* coord, int64_t n_links, int64_t n_points, bool geographic, NetRows& out, std::string& err);
// the layer of 17 fields with the reference's widths and decimals, one line per link
void net_layer(const int64_t* tree, int64_t n_links, const NetRows& rows, tdx::LineLayer& layer);

}  // namespace streamnet
