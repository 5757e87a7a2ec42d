// CatchOutlets (src/CatchOutlets.cpp:87-443): outlets along a stream network, one at the downstream end of every outlet link and one at the upstream end
// of every link that lies more than mindist above the last outlet written below it and drains more than minarea.  Host code - a tree walk over the link
// table and one cell of p per outlet link - without HIP headers or a context: tests/netlayer/netlayer_main.cpp builds the same file.
#pragma once
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "vector_layer.hpp"

namespace tdx {

struct NetLink {
    int32_t linkno = 0, dslinkno = 0, uslinkno1 = 0, uslinkno2 = 0;
    double doutend = 0, doutstart = 0, uscontarea = 0;
    double down_x = 0, down_y = 0, up_x = 0, up_y = 0;   // the link's downstream and upstream end
};
struct CatchOutlet {
    int64_t row = 0;      // the link's place in the table
    double x = 0, y = 0;
    double doutend = 0;   // the DOUTEND field: the link's DOUTEND on an outlet link, its DOUTSTART on every other (src/CatchOutlets.cpp:306, :311)
    int32_t id = 0;
};
// where the raster lies (tiffIO::geoToGlobalXY / globalXYToGeo) and how a cell of p is had: false = it could not be read
struct FlowGrid {
    int64_t nx = 0, ny = 0;
    double xleftedge = 0, ytopedge = 0, dlon = 1, dlat = 1;
    std::function<bool(int64_t col, int64_t row, int16_t& dir)> p_at;
};

// From a line layer: LINKNO, DSLINKNO, USLINKNO1, USLINKNO2, DOUTEND, DOUTSTART, USContArea by name (the first missing one is named in err); vertex 0 is
// the downstream end, the last vertex the upstream end.  A link that is kept (below) must have a vertex.
bool links_from_layer(const LineLayer& layer, std::vector<NetLink>& links, std::string& err);
// From this project's streamnet -tree and -coord files, values as the text holds them: DOUTEND and the downstream end from the link's last coord row,
// DOUTSTART, USContArea and the upstream end from its first.
bool links_from_text(const std::string& treefile, const std::string& coordfile, std::vector<NetLink>& links, std::string& err);

// The outlets in the reference's order of writing.  false: a cell of p could not be read, or the upstream links close a cycle (the reference would recurse
// without end).  The walk keeps its own stack: a chain of any length is walked.
bool catch_outlets(const std::vector<NetLink>& links, const FlowGrid& grid, double mindist, int32_t gwstartno, double minarea, std::vector<CatchOutlet>& out,
                   std::string& err);
// the point layer of the reference: LINKNO, DSLINKNO, USLINKNO1, USLINKNO2 (Integer 6), DOUTEND (Real 16.1), Id (Integer 10)
void catch_outlets_layer(const std::vector<NetLink>& links, const std::vector<CatchOutlet>& outlets, PointLayer& layer);

}  // namespace tdx
