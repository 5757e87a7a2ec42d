// The host ring builder: the default, and the witness of the device ring builder (polygon_rings_device.hip), which must make the same arrays of the
// same edges and refuse the same edges for the same reasons.  The tests hold the two against each other and both against tests/polygonize_model.py.
#include "polygon_rings.hpp"

#include <algorithm>
#include <tuple>

namespace polygons {
namespace {

// start vertex of the edge `side` of cell (c, r)
inline void edge_start(int64_t c, int64_t r, int side, int64_t& vc, int64_t& vr) {
    vc = c + ((side == 1 || side == 2) ? 1 : 0);
    vr = r + ((side == 2 || side == 3) ? 1 : 0);
}
inline void edge_end(int64_t c, int64_t r, int side, int64_t& vc, int64_t& vr) { edge_start(c, r, (side + 1) & 3, vc, vr); }

struct Ring {
    int64_t r0, c0;      // start vertex
    int64_t area2;       // shoelace sum: twice the signed area, positive for an outer ring
    int64_t first, last; // its vertices in the walk's list, closed
    int32_t id;
    int64_t owner;       // hole: its outer ring; outer ring: itself
};

struct Edges {
    const int64_t* key = nullptr;
    const int64_t* next = nullptr;
    const int32_t* id = nullptr;
    int64_t n = 0, nx = 0, ny = 0;
    std::vector<int64_t> row_first;   // [ny + 1] the first edge of every row
    // index of the edge with key k, or -1
    int64_t find(int64_t k) const {
        if (k < 0) return -1;
        const int64_t r = k / (4 * nx);
        if (r >= ny) return -1;
        const int64_t* a = key + row_first[size_t(r)];
        const int64_t* b = key + row_first[size_t(r) + 1];
        const int64_t* it = std::lower_bound(a, b, k);
        return (it != b && *it == k) ? int64_t(it - key) : -1;
    }
};

}  // namespace

bool build_rings(const EdgePart* const* parts, size_t n_parts, int64_t nx, int64_t ny, Polygons& out, std::string& err) {
    out = Polygons();
    if (nx <= 0 || ny <= 0 || (n_parts > 0 && !parts)) { err = "polygon rings: bad argument"; return false; }
    // ---- the parts as one list
    EdgePart joined;
    Edges E;
    E.nx = nx; E.ny = ny;
    size_t total = 0;
    for (size_t k = 0; k < n_parts; k++) {
        if (!parts[k] || parts[k]->key.size() != parts[k]->next.size() || parts[k]->key.size() != parts[k]->id.size()) { err = "polygon rings: a part with columns of different length"; return false; }
        total += parts[k]->key.size();
    }
    if (n_parts == 1) { E.key = parts[0]->key.data(); E.next = parts[0]->next.data(); E.id = parts[0]->id.data(); }
    else {
        joined.key.reserve(total); joined.next.reserve(total); joined.id.reserve(total);
        for (size_t k = 0; k < n_parts; k++) {
            joined.key.insert(joined.key.end(), parts[k]->key.begin(), parts[k]->key.end());
            joined.next.insert(joined.next.end(), parts[k]->next.begin(), parts[k]->next.end());
            joined.id.insert(joined.id.end(), parts[k]->id.begin(), parts[k]->id.end());
        }
        E.key = joined.key.data(); E.next = joined.next.data(); E.id = joined.id.data();
    }
    E.n = int64_t(total);
    if (nx > (INT64_MAX / 4) / ny) { err = "polygon rings: raster too large for 64-bit keys"; return false; }
    const int64_t key_end = nx * ny * 4;
    E.row_first.assign(size_t(ny) + 1, E.n);
    {
        int64_t row = 0;
        for (int64_t e = 0; e < E.n; e++) {
            const int64_t k = E.key[e];
            if (k < 0 || k >= key_end) { err = "polygon rings: an edge key outside the raster"; return false; }
            if (e > 0 && k <= E.key[e - 1]) { err = "polygon rings: edge keys do not ascend (parts out of order?)"; return false; }
            const int64_t r = k / (4 * nx);
            while (row <= r) E.row_first[size_t(row++)] = e;
        }
    }
    // ---- the cycles
    std::vector<int64_t> ring_of(size_t(E.n), -1);
    std::vector<Ring> rings;
    std::vector<int32_t> walk;   // column, row of every ring's vertices, closed
    std::vector<int32_t> v;
    for (int64_t e0 = 0; e0 < E.n; e0++) {
        if (ring_of[size_t(e0)] >= 0) continue;
        const int64_t R = int64_t(rings.size());
        const int32_t id = E.id[e0];
        v.clear();
        int prev_side = -1;
        const int first_side = int(E.key[e0] & 3);
        int64_t e = e0;
        for (;;) {
            ring_of[size_t(e)] = R;
            if (E.id[e] != id) { err = "polygon rings: the id changes along a ring"; return false; }
            const int64_t cell = E.key[e] >> 2;
            const int side = int(E.key[e] & 3);
            const int64_t c = cell % nx, r = cell / nx;
            if (prev_side >= 0 && side != prev_side) {
                int64_t vc, vr;
                edge_start(c, r, side, vc, vr);
                v.push_back(int32_t(vc)); v.push_back(int32_t(vr));
            }
            prev_side = side;
            const int64_t nxt = E.find(E.next[e]);
            if (nxt < 0) { err = "polygon rings: the successor of an edge is not among the edges (a strip missing, or parts out of order?)"; return false; }
            {   // the successor starts where the edge ends
                int64_t ec, er, sc, sr;
                edge_end(c, r, side, ec, er);
                const int64_t ncell = E.key[nxt] >> 2;
                edge_start(ncell % nx, ncell / nx, int(E.key[nxt] & 3), sc, sr);
                if (ec != sc || er != sr) { err = "polygon rings: a successor does not start where its edge ends"; return false; }
            }
            if (nxt == e0) break;
            if (ring_of[size_t(nxt)] >= 0) { err = "polygon rings: the successors are not a permutation of the edges"; return false; }
            e = nxt;
        }
        if (prev_side != first_side) {
            const int64_t cell = E.key[e0] >> 2;
            int64_t vc, vr;
            edge_start(cell % nx, cell / nx, first_side, vc, vr);
            v.push_back(int32_t(vc)); v.push_back(int32_t(vr));
        }
        const size_t nv = v.size() / 2;
        if (nv < 4) { err = "polygon rings: a ring of fewer than four corners"; return false; }
        size_t s = 0;
        for (size_t i = 1; i < nv; i++)
            if (std::make_pair(v[2 * i + 1], v[2 * i]) < std::make_pair(v[2 * s + 1], v[2 * s])) s = i;
        Ring G;
        G.id = id; G.c0 = v[2 * s]; G.r0 = v[2 * s + 1]; G.first = int64_t(walk.size() / 2); G.owner = R;
        int64_t a2 = 0;
        for (size_t i = 0; i <= nv; i++) {
            const size_t j = (s + i) % nv;
            walk.push_back(v[2 * j]); walk.push_back(v[2 * j + 1]);
            if (i < nv) {
                const size_t j1 = (j + 1) % nv;
                a2 += int64_t(v[2 * j]) * int64_t(v[2 * j1 + 1]) - int64_t(v[2 * j1]) * int64_t(v[2 * j + 1]);
            }
        }
        G.last = int64_t(walk.size() / 2);
        G.area2 = a2;
        if (a2 == 0) { err = "polygon rings: a ring without area"; return false; }
        rings.push_back(G);
    }
    // ---- holes to their outer rings, in ascending order of start vertex
    std::vector<int64_t> holes;
    for (size_t q = 0; q < rings.size(); q++)
        if (rings[q].area2 < 0) { holes.push_back(int64_t(q)); rings[q].owner = -1; }
    auto by_start = [&](int64_t a, int64_t b) { return std::tie(rings[size_t(a)].r0, rings[size_t(a)].c0) < std::tie(rings[size_t(b)].r0, rings[size_t(b)].c0); };
    std::sort(holes.begin(), holes.end(), by_start);
    for (int64_t h : holes) {
        Ring& H = rings[size_t(h)];
        int64_t owner = -1;
        if (H.c0 < nx)
            for (int64_t r = H.r0 - 1; r >= 0; r--) {   // up the column to the first cell whose top side is a boundary edge
                const int64_t e = E.find((r * nx + H.c0) * 4);
                if (e < 0) continue;
                const Ring& Q = rings[size_t(ring_of[size_t(e)])];
                if (Q.id == H.id) owner = Q.owner;
                break;
            }
        if (owner < 0) { err = "polygon rings: a hole without an outer ring"; return false; }
        H.owner = owner;
    }
    // ---- the layer
    std::vector<int64_t> order(rings.size());
    for (size_t q = 0; q < rings.size(); q++) order[q] = int64_t(q);
    // feature by id, polygon by the outer ring's start vertex, the outer ring before its holes, holes by start vertex
    std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
        const Ring &A = rings[size_t(a)], &B = rings[size_t(b)];
        const Ring &OA = rings[size_t(A.owner)], &OB = rings[size_t(B.owner)];
        const int ha = A.area2 < 0, hb = B.area2 < 0;
        return std::tie(A.id, OA.r0, OA.c0, ha, A.r0, A.c0) < std::tie(B.id, OB.r0, OB.c0, hb, B.r0, B.c0);
    });
    out.poly_first.push_back(0);
    out.ring_first.push_back(0);
    out.vert_first.push_back(0);
    out.vert.reserve(walk.size());
    for (size_t i = 0; i < order.size(); i++) {
        const Ring& G = rings[size_t(order[i])];
        const bool outer = G.area2 > 0;
        if (outer) {   // a new polygon, and with a new id a new feature
            if (i > 0) out.ring_first.push_back(int64_t(out.vert_first.size()) - 1);
            if (out.id.empty() || out.id.back() != G.id) {
                if (!out.id.empty()) out.poly_first.push_back(int64_t(out.ring_first.size()) - 1);
                out.id.push_back(G.id);
                out.cells.push_back(0);
            }
        }
        out.cells.back() += G.area2;
        out.vert.insert(out.vert.end(), walk.begin() + 2 * G.first, walk.begin() + 2 * G.last);
        out.vert_first.push_back(int64_t(out.vert.size() / 2));
    }
    if (!order.empty()) {
        out.ring_first.push_back(int64_t(out.vert_first.size()) - 1);
        out.poly_first.push_back(int64_t(out.ring_first.size()) - 1);
    } else {
        out.ring_first.assign(1, 0);
    }
    for (int64_t& c : out.cells) c /= 2;
    return true;
}

}  // namespace polygons
