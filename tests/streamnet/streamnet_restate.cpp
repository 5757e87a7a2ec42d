/* A serial restatement of StreamNet (netsetup, src/streamnet.cpp:372-1508, with the link set of src/linklib.h) on one rank, written from the
 * rules of DESIGN.md section "StreamNet": whole-raster grids, literal FIFO queues, one std::vector of points per link.  It is the checker at sizes
 * the reference goldens do not cover; tests/test_streamnet_restatement.py holds it to every golden byte.  Built by the tests with
 * `c++ -O2 -ffp-contract=off -shared -fPIC`.
 *
 * Cells off the raster read as nodata everywhere (one rank: the border rows hold nodata).  A direction code outside 0..8 is undefined in the
 * reference (it indexes d1 / d2); here such a cell has no receiver and points at nobody.  p == 0 points at the cell itself. */
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <deque>
#include <vector>

namespace {
const int DX_[9] = {0, 1, 1, 0, -1, -1, -1, 0, 1};
const int DY_[9] = {0, 0, -1, -1, -1, 0, 1, 1, 1};
const int32_t LONG_ND = -2147483647;   // MISSINGLONG
const int16_t SHORT_ND = -32768;       // MISSINGSHORT
const float FLOAT_ND = -FLT_MAX;       // MISSINGFLOAT

struct Point { long x, y; float elev, area, length; };
struct Link {
    int32_t id, u1, u2;
    long d, magnitude, shape;
    short order;
    std::vector<Point> pts;
};

struct Grid {
    int nx, ny;
    const int16_t* p; int16_t p_nd;
    const int32_t* src; int32_t src_nd;
    bool in(long x, long y) const { return x >= 0 && x < nx && y >= 0 && y < ny; }
    size_t at(long x, long y) const { return size_t(y) * size_t(nx) + size_t(x); }
    bool p_valid(long x, long y) const { return in(x, y) && p[at(x, y)] != p_nd; }
    bool src_pos(long x, long y) const { return in(x, y) && src[at(x, y)] != src_nd && src[at(x, y)] > 0; }
    bool stream(long x, long y) const { return src_pos(x, y) && p_valid(x, y); }
    // the receiver of a cell with a direction value; false: the code points nowhere
    bool recv(long x, long y, long& xr, long& yr) const {
        const int k = p[at(x, y)];
        if (k < 0 || k > 8) return false;
        xr = x + DX_[k]; yr = y + DY_[k];
        return true;
    }
    bool points_to_me(long x, long y, long xn, long yn) const {   // src/streamnet.cpp:97-105
        if (!p_valid(xn, yn)) return false;
        long xr = -1, yr = -1;
        return recv(xn, yn, xr, yr) && xr == x && yr == y;
    }
};

std::vector<int64_t> g_tree;
std::vector<double> g_coord;
std::vector<int64_t> g_ci;      // compact arrays of the last run (the stream cells in row-major order)
std::vector<int16_t> g_cp;
std::vector<float> g_cfel, g_cad8, g_clen;
std::vector<int32_t> g_cout, g_crecv;
std::vector<uint8_t> g_cflag;
}  // namespace

extern "C" {

/* gt: {x of the left edge, cell width, y of the top edge, cell height} of the raster file.  Outlets: global column / row and id.  sw != 0: -sw.
 * Outputs: ord (int16, nodata -32768), w (int32, nodata MISSINGLONG); n_links / n_points for sn_fetch.  Returns 0. */
int sn_run(int nx, int ny, const int16_t* p, int16_t p_nd, const int32_t* src, int32_t src_nd, const float* fel, const float* ad8, const double* dxc,
           const double* dyc, double dxA, double dyA, const double* gt, int nout, const int32_t* ox, const int32_t* oy, const int32_t* oid, int sw, int16_t* ord,
           int32_t* w, int64_t* n_links, int64_t* n_points) {
    const Grid G{nx, ny, p, p_nd, src, src_nd};
    const size_t n = size_t(nx) * size_t(ny);
    std::vector<int32_t> idGrid(n, LONG_ND), wsGrid(n, LONG_ND);
    std::vector<int16_t> contribs(n, SHORT_ND);
    std::vector<float> lengths(n, FLOAT_ND);
    std::vector<Link> links;
    std::deque<size_t> que;

    for (int o = 0; o < nout; o++)   // :514-521, the last outlet on a cell wins
        if (G.in(ox[o], oy[o])) idGrid[G.at(ox[o], oy[o])] = oid[o];

    // ---- distance to the outlet along the stream (:562-650)
    for (long j = 0; j < ny; j++)
        for (long i = 0; i < nx; i++) {
            if (!G.stream(i, j)) continue;
            long xr = -1, yr = -1;
            if (G.recv(i, j, xr, yr) && G.stream(xr, yr)) contribs[G.at(i, j)] = 1;
            else { contribs[G.at(i, j)] = 0; que.push_back(G.at(i, j)); }
        }
    while (!que.empty()) {
        const size_t c = que.front();
        que.pop_front();
        const long i = long(c % size_t(nx)), j = long(c / size_t(nx));
        const int k = p[c];
        float llength = 0.f;
        long xr = -1, yr = -1;
        if (G.recv(i, j, xr, yr) && G.in(xr, yr) && lengths[G.at(xr, yr)] != FLOAT_ND) {
            llength += lengths[G.at(xr, yr)];
            if (k == 1 || k == 5) llength = llength + dxc[j];
            if (k == 3 || k == 7) llength = llength + dyc[j];
            if (k % 2 == 0) llength = llength + sqrt(dxc[j] * dxc[j] + dyc[j] * dyc[j]);
        }
        lengths[c] = llength;
        for (int m = 1; m <= 8; m++) {
            const long xn = i + DX_[m], yn = j + DY_[m];
            if (G.points_to_me(i, j, xn, yn) && G.src_pos(xn, yn)) {
                int16_t& cn = contribs[G.at(xn, yn)];
                cn = int16_t(cn - 1);
                if (cn == 0) que.push_back(G.at(xn, yn));
            }
        }
    }
    g_ci.clear(); g_cp.clear(); g_cfel.clear(); g_cad8.clear(); g_clen.clear(); g_cout.clear(); g_crecv.clear(); g_cflag.clear();
    {   // the compact arrays the product's host link builder works on (dumped for its stand-alone check)
        std::vector<int32_t> rank(n, -1);
        int32_t r = 0;
        for (size_t c = 0; c < n; c++) if (G.stream(long(c % size_t(nx)), long(c / size_t(nx)))) rank[c] = r++;
        for (size_t c = 0; c < n; c++) {
            if (rank[c] < 0) continue;
            const long i = long(c % size_t(nx)), j = long(c / size_t(nx));
            long xr = -1, yr = -1;
            const bool has = G.recv(i, j, xr, yr);
            g_ci.push_back(int64_t(c)); g_cp.push_back(p[c]); g_cfel.push_back(fel[c]); g_cad8.push_back(ad8[c]); g_clen.push_back(lengths[c]);
            g_cout.push_back(idGrid[c]);
            g_crecv.push_back(has && G.stream(xr, yr) ? rank[G.at(xr, yr)] : -1);
            g_cflag.push_back(uint8_t(!has || !G.in(xr, yr) || src[G.at(xr, yr)] == src_nd || src[G.at(xr, yr)] != 1));
        }
    }

    // ---- links (:668-959)
    std::fill(contribs.begin(), contribs.end(), SHORT_ND);
    for (long j = 0; j < ny; j++)
        for (long i = 0; i < nx; i++) {
            if (!G.stream(i, j)) continue;
            int16_t tempc = 0;
            for (int m = 1; m <= 8; m++)
                if (G.points_to_me(i, j, i + DX_[m], j + DY_[m]) && G.src_pos(i + DX_[m], j + DY_[m])) tempc++;
            contribs[G.at(i, j)] = tempc;
            if (tempc == 0) que.push_back(G.at(i, j));
        }
    auto create = [&](int32_t u1, int32_t u2, const Point& pt) -> int32_t {   // src/linklib.h:436-485
        Link L;
        L.id = int32_t(links.size()); L.u1 = u1; L.u2 = u2; L.d = -1; L.magnitude = 1; L.shape = -1; L.order = 1;
        L.pts.push_back(pt);
        links.push_back(L);
        return L.id;
    };
    while (!que.empty()) {
        const size_t c = que.front();
        que.pop_front();
        const long i = long(c % size_t(nx)), j = long(c / size_t(nx));
        short nOrder[8], inneighbors[8];
        long k = 0;
        for (int m = 1; m <= 8; m++) {
            const long xn = i + DX_[m], yn = j + DY_[m];
            if (G.points_to_me(i, j, xn, yn) && G.src_pos(xn, yn) && idGrid[G.at(xn, yn)] != LONG_ND) {
                inneighbors[k] = short(m);
                nOrder[k] = short(lengths[G.at(xn, yn)]);
                k++;
            }
        }
        long xr = -1, yr = -1;
        const bool has = G.recv(i, j, xr, yr);
        const bool mandatory = idGrid[c] != LONG_ND;
        const int32_t shapeID = idGrid[c];
        const bool terminal = !has || !G.in(xr, yr) || src[G.at(xr, yr)] == src_nd || src[G.at(xr, yr)] != 1;
        const Point pt{i, j, fel[c], ad8[c], lengths[c]};
        auto id_of = [&](int a) { return idGrid[G.at(i + DX_[inneighbors[a]], j + DY_[inneighbors[a]])]; };
        if (k == 0) {
            const int32_t u1 = create(-1, -1, pt);
            idGrid[c] = u1; wsGrid[c] = u1; lengths[c] = float(links[u1].order);
            if (mandatory) {
                links[u1].pts.push_back(pt);
                links[u1].shape = shapeID;
                if (!terminal) {
                    const int32_t nl = create(u1, -1, pt);
                    links[nl].order = 1; links[u1].d = nl; links[nl].magnitude = 1;
                    idGrid[c] = nl;
                }
            } else if (terminal) links[u1].pts.push_back(pt);
        } else if (k == 1) {
            const int32_t u1 = id_of(0);
            links[u1].pts.push_back(pt);
            idGrid[c] = u1; wsGrid[c] = u1; lengths[c] = float(nOrder[0]);
            if (mandatory) {
                links[u1].shape = shapeID;
                if (!terminal) {
                    const int32_t nl = create(u1, -1, pt);
                    links[nl].order = links[u1].order; links[u1].d = nl; links[nl].magnitude = links[u1].magnitude;
                    idGrid[c] = nl;
                }
            }
        } else {
            for (int a = 0; a < 2; ++a)   // :839-851, exactly as written
                for (int b = 0; b < k - 1; ++b)
                    if (nOrder[b] > nOrder[b + 1]) {
                        short t = nOrder[b]; nOrder[b] = nOrder[b + 1]; nOrder[b + 1] = t;
                        t = inneighbors[b]; inneighbors[b] = inneighbors[b + 1]; inneighbors[b + 1] = t;
                    }
            const short oOut = nOrder[k - 2] == nOrder[k - 1] ? short(nOrder[k - 1] + 1) : nOrder[k - 1];
            int32_t u1 = id_of(int(k - 1)), u2 = id_of(int(k - 2));
            links[u1].pts.push_back(pt);
            links[u2].pts.push_back(pt);
            int32_t nl = create(u1, u2, pt);
            links[nl].order = oOut; links[u1].d = nl; links[u2].d = nl;
            links[nl].magnitude = links[u1].magnitude + links[u2].magnitude;
            for (long m = 2; m < k; m++) {
                u1 = nl;
                u2 = id_of(int(k - m - 1));
                links[u1].pts.push_back(pt);
                links[u2].pts.push_back(pt);
                nl = create(u1, u2, pt);
                links[nl].order = oOut; links[u1].d = nl; links[u2].d = nl;
                links[nl].magnitude = links[u1].magnitude + links[u2].magnitude;
            }
            idGrid[c] = nl; wsGrid[c] = nl; lengths[c] = float(oOut);
            if (mandatory) {
                u1 = nl;
                links[u1].pts.push_back(pt);
                links[u1].shape = shapeID;
                if (!terminal) {
                    nl = create(u1, -1, pt);
                    links[nl].order = oOut; links[u1].d = nl; links[nl].magnitude = links[u1].magnitude;
                    idGrid[c] = nl;
                }
            } else if (terminal) links[nl].pts.push_back(pt);
        }
        if (has && G.in(xr, yr)) {
            int16_t& cr = contribs[G.at(xr, yr)];
            cr = int16_t(cr - 1);
            if (cr == 0) que.push_back(G.at(xr, yr));
        }
    }

    // ---- tree and coord rows (src/linklib.h:800-846, :1164-1183): the link set is a list with insertion at the head
    g_tree.clear(); g_coord.clear();
    const double cellarea = dxA * dyA;
    long beg = 0;
    for (size_t a = links.size(); a-- > 0;) {
        const Link& L = links[a];
        const long end = beg + long(L.pts.size()) - 1;
        const int64_t row[9] = {L.id, beg, end, L.d, L.u1, L.u2, L.order, L.shape, L.magnitude};
        g_tree.insert(g_tree.end(), row, row + 9);
        for (const Point& q : L.pts) {
            const float area = q.area * cellarea;
            g_coord.push_back(gt[0] + gt[1] / 2. + q.x * gt[1]);
            g_coord.push_back(gt[2] - gt[3] / 2. - q.y * gt[3]);
            g_coord.push_back(q.length);
            g_coord.push_back(q.elev);
            g_coord.push_back(area);
        }
        beg = end + 1;
    }
    *n_links = int64_t(links.size());
    *n_points = int64_t(g_coord.size() / 5);

    // ---- watersheds (:1344-1441)
    std::fill(contribs.begin(), contribs.end(), SHORT_ND);
    for (long j = 0; j < ny; j++)
        for (long i = 0; i < nx; i++) {
            const size_t c = G.at(i, j);
            if (p[c] == p_nd) continue;
            if (src[c] == src_nd || src[c] < 1) {
                long xr = -1, yr = -1;
                if (!G.recv(i, j, xr, yr) || !G.in(xr, yr)) continue;
                const size_t r = G.at(xr, yr);
                if (src[r] == src_nd || src[r] < 1) { contribs[c] = 1; wsGrid[c] = LONG_ND; }
                else { contribs[c] = 0; que.push_back(c); }
            } else if (sw) wsGrid[c] = 1;
        }
    while (!que.empty()) {
        const size_t c = que.front();
        que.pop_front();
        const long i = long(c % size_t(nx)), j = long(c / size_t(nx));
        long xr = -1, yr = -1;
        G.recv(i, j, xr, yr);
        wsGrid[c] = sw ? 1 : wsGrid[G.at(xr, yr)];
        for (int m = 1; m <= 8; m++) {
            const long xn = i + DX_[m], yn = j + DY_[m];
            if (!G.points_to_me(i, j, xn, yn)) continue;
            int16_t& cn = contribs[G.at(xn, yn)];
            cn = int16_t(cn - 1);
            if (cn == 0) que.push_back(G.at(xn, yn));
        }
    }
    for (size_t c = 0; c < n; c++) {   // :1460-1474
        w[c] = wsGrid[c];
        ord[c] = lengths[c] != FLOAT_ND ? int16_t(lengths[c]) : int16_t(0);
    }
    return 0;
}

void sn_fetch(int64_t* tree, double* coord) {
    if (!g_tree.empty()) memcpy(tree, g_tree.data(), g_tree.size() * sizeof(int64_t));
    if (!g_coord.empty()) memcpy(coord, g_coord.data(), g_coord.size() * sizeof(double));
}

/* The compact arrays of the last run as one binary file: int64 n, then idx[n] p[n] fel[n] ad8[n] len[n] outlet[n] recv[n] flags[n]. */
int sn_dump_compact(const char* path) {
    FILE* f = fopen(path, "wb");
    if (!f) return -1;
    const int64_t n = int64_t(g_ci.size());
    fwrite(&n, 8, 1, f);
    fwrite(g_ci.data(), 8, size_t(n), f); fwrite(g_cp.data(), 2, size_t(n), f); fwrite(g_cfel.data(), 4, size_t(n), f); fwrite(g_cad8.data(), 4, size_t(n), f);
    fwrite(g_clen.data(), 4, size_t(n), f); fwrite(g_cout.data(), 4, size_t(n), f); fwrite(g_crecv.data(), 4, size_t(n), f); fwrite(g_cflag.data(), 1, size_t(n), f);
    return fclose(f);
}
}
