// Watershed polygons: the boundary edges of an id grid (polygonize.hip makes them on the device, sorted by key) closed into rings, the rings sorted
// into outer rings and holes, and everything ordered into the layer.  Plain C++, no HIP headers.
//   edge key    (r * nx + c) * 4 + side of the cell (c, r) that carries the edge; side 0 top, 1 right, 2 bottom, 3 left, the id on the right of the
//               direction of travel: top (c, r) -> (c + 1, r), right (c + 1, r) -> (c + 1, r + 1), bottom (c + 1, r + 1) -> (c, r + 1), left (c, r + 1) -> (c, r)
//   successor   the key of the boundary edge of the same id that starts where the edge ends (the one that turns right where there are two)
//   ring        a cycle of the successor map: only the vertices at which the direction changes, from its smallest vertex by (r, c), closed
//   outer ring  positive shoelace area in (c, r), which is clockwise in map view; a hole of id a that starts at (c0, r0) belongs to the piece of a
//               that holds the cell (c0, r0 - 1)
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace polygons {

struct EdgePart {   // the edges of a run of rows, ascending by key
    std::vector<int64_t> key, next;
    std::vector<int32_t> id;
};

// features -> polygons -> rings -> vertices as offset lists
struct Polygons {
    std::vector<int32_t> id;          // [features] ascending
    std::vector<int64_t> cells;       // [features] half the sum of the signed shoelace areas of the feature's rings = the cells that hold the id
    std::vector<int64_t> poly_first;  // [features + 1] polygons of a feature, ordered by the start vertex of their outer ring
    std::vector<int64_t> ring_first;  // [polygons + 1] rings of a polygon: the outer ring, then its holes by start vertex
    std::vector<int64_t> vert_first;  // [rings + 1]
    std::vector<int32_t> vert;        // [vertices][2] column, row; a ring repeats its first vertex at its end
    size_t features() const { return id.size(); }
    size_t n_polygons() const { return ring_first.empty() ? 0 : ring_first.size() - 1; }
    size_t n_rings() const { return vert_first.empty() ? 0 : vert_first.size() - 1; }
    size_t n_vertices() const { return vert.size() / 2; }
};

// The parts of ALL strips in strip order, which is key order.  false + err: keys that do not ascend (parts out of order), a key outside the raster,
// a successor that is not among the keys (a strip is missing), an id that changes along a ring.
bool build_rings(const EdgePart* const* parts, size_t n_parts, int64_t nx, int64_t ny, Polygons& out, std::string& err);

}  // namespace polygons
