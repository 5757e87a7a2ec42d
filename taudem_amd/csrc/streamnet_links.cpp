// StreamNet's link builder on the host: see streamnet_links.hpp.  The reference's queue is a literal FIFO and its link numbers come from one
// counter in the order the queue pops (src/linklib.h:445-450), so the walk below IS the definition of the numbering on one rank.
//
// A link's points are never stored while the walk runs.  Every point a link receives is the cell being processed, and that cell is either the
// receiver of the link's last cell (appendPoint at the next cell down: :807, :863-864, :883-884) or the cell the link was created on, once more
// (mandatory junctions, terminal links and the inner links of a k >= 3 junction: :784, :800, :883, :906, :922).  So a link is its first cell, whether
// that cell is doubled, and a count; the points come out at the end by following `recv`, straight into the one coord array whose row ranges the
// tree rows hold.
#include "streamnet_links.hpp"

#include <cstddef>

namespace streamnet {
namespace {
struct Link {
    int32_t u1, u2;
    int64_t d, magnitude, shape;
    int32_t first;      // compact rank of the first point
    int32_t count;      // numCoords
    int16_t order;
    bool doubled;       // the first cell is also the second point
};
}  // namespace

void build_links(const Compact& C, int64_t nx, double dxA, double dyA, const double* gt, Links& out) {
    const size_t n = size_t(C.n);
    out.tree.clear(); out.coord.clear();
    out.label.assign(n, LINK_NONE);
    out.order.assign(n, 0);
    // inflows by neighbour number m = 1..8 as seen from the receiver (the order of the loop at :736-745): a cell with code k lies at m = k + 4 (mod 8).
    // p == 0 names the cell itself, which the neighbour loop never visits.
    std::vector<int32_t> inflow(n * 8, -1), waiting(n, 0), queue, id(C.outlet, C.outlet + n);
    for (size_t u = 0; u < n; u++) {
        const int32_t r = C.recv[u];
        const int k = C.p[u];
        if (r < 0 || size_t(r) == u || k < 1 || k > 8) continue;
        inflow[size_t(r) * 8 + size_t((k - 1 + 4) % 8)] = int32_t(u);
        waiting[size_t(r)]++;
    }
    queue.reserve(n);
    for (size_t c = 0; c < n; c++) if (waiting[c] == 0) queue.push_back(int32_t(c));
    std::vector<Link> links;
    auto create = [&](int32_t u1, int32_t u2, int32_t c) -> int32_t {   // src/linklib.h:436-485
        links.push_back(Link{u1, u2, -1, 1, -1, c, 1, 1, false});
        return int32_t(links.size() - 1);
    };
    auto append_next = [&](int32_t u) { links[size_t(u)].count++; };
    auto append_again = [&](int32_t u) { links[size_t(u)].count++; links[size_t(u)].doubled = true; };
    for (size_t head = 0; head < queue.size(); head++) {
        const int32_t c = queue[head];
        int16_t nOrder[8], from[8];
        int k = 0;
        for (int m = 0; m < 8; m++) {
            const int32_t u = inflow[size_t(c) * 8 + size_t(m)];
            if (u < 0 || id[size_t(u)] == LINK_NONE) continue;
            from[k] = int16_t(m);
            nOrder[k] = out.order[size_t(u)];
            k++;
        }
        auto id_of = [&](int a) { return id[size_t(inflow[size_t(c) * 8 + size_t(from[a])])]; };
        const bool mandatory = id[size_t(c)] != LINK_NONE, terminal = (C.flags[c] & CELL_TERMINAL) != 0;
        const int32_t shape = id[size_t(c)];
        int32_t last;      // the link that ends or goes on at this cell: wsGrid
        int16_t oOut;
        if (k == 0) {
            last = create(-1, -1, c);
            oOut = 1;
            if (!mandatory && terminal) append_again(last);
        } else if (k == 1) {
            last = id_of(0);
            append_next(last);
            oOut = nOrder[0];
        } else {
            for (int a = 0; a < 2; ++a)   // :839-851 exactly as written: two bubble passes, whose tie order decides u1 and u2
                for (int b = 0; b < k - 1; ++b)
                    if (nOrder[b] > nOrder[b + 1]) {
                        int16_t t = nOrder[b]; nOrder[b] = nOrder[b + 1]; nOrder[b + 1] = t;
                        t = from[b]; from[b] = from[b + 1]; from[b + 1] = t;
                    }
            oOut = nOrder[k - 2] == nOrder[k - 1] ? int16_t(nOrder[k - 1] + 1) : nOrder[k - 1];
            int32_t u1 = id_of(k - 1);
            for (int m = 2; m <= k; m++) {   // the links of a k >= 3 junction are chained: the new link is the next one's u1
                const int32_t u2 = id_of(k - m);
                if (m == 2) append_next(u1); else append_again(u1);
                append_next(u2);
                const int32_t nl = create(u1, u2, c);
                Link& L = links[size_t(nl)];
                L.order = oOut;
                L.magnitude = links[size_t(u1)].magnitude + links[size_t(u2)].magnitude;
                links[size_t(u1)].d = nl;
                links[size_t(u2)].d = nl;
                u1 = nl;
            }
            last = u1;
            if (!mandatory && terminal) append_again(last);
        }
        id[size_t(c)] = last;
        out.label[size_t(c)] = last;
        out.order[size_t(c)] = oOut;
        if (mandatory) {   // the link ends here with the outlet's id; below it a new link of the same order and magnitude (:782-798, :817-830, :903-919)
            if (k != 1) append_again(last);
            links[size_t(last)].shape = shape;
            if (!terminal) {
                const int32_t nl = create(last, -1, c);
                links[size_t(nl)].order = links[size_t(last)].order;
                links[size_t(nl)].magnitude = links[size_t(last)].magnitude;
                links[size_t(last)].d = nl;
                id[size_t(c)] = nl;   // idGrid and wsGrid deliberately out of step (:794-797): the next cell down continues the new link
            }
        }
        const int32_t r = C.recv[c];
        if (r >= 0 && r != c && --waiting[size_t(r)] == 0) queue.push_back(r);
    }

    // rows in the order of the reference's list, which inserts at its head: the last link first
    const double cellarea = dxA * dyA;
    size_t npts = 0;
    for (const Link& L : links) npts += size_t(L.count);
    out.tree.reserve(links.size() * 9);
    out.coord.reserve(npts * 5);
    int64_t beg = 0;
    for (size_t a = links.size(); a-- > 0;) {
        const Link& L = links[a];
        const int64_t end = beg + L.count - 1;
        const int64_t row[9] = {int64_t(a), beg, end, L.d, L.u1, L.u2, L.order, L.shape, L.magnitude};
        out.tree.insert(out.tree.end(), row, row + 9);
        int32_t c = L.first;
        for (int32_t i = 0; i < L.count; i++) {
            const int64_t x = C.idx[c] % nx, y = C.idx[c] / nx;
            const float area = C.ad8[c] * cellarea;   // float * double, stored as float (src/linklib.h:836)
            const double pt[5] = {gt[0] + gt[1] / 2. + x * gt[1], gt[2] - gt[3] / 2. - y * gt[3], C.len[c], C.fel[c], area};
            out.coord.insert(out.coord.end(), pt, pt + 5);
            if (!(i == 0 && L.doubled) && i + 1 < L.count) c = C.recv[c];
        }
        beg = end + 1;
    }
}

}  // namespace streamnet
