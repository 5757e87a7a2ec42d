#include "streamnet_net.hpp"

#include <cmath>

#include "geo_length.hpp"

namespace streamnet {
namespace {

// the length of the step (dx, dy) that ends at latitude y (src/streamnet.cpp:281-289, :306-315)
double step_length(double dx, double dy, double y, bool geographic) {
    if (!geographic) return sqrt(dx * dx + dy * dy);
    double d[2];
    tdx::geo_to_length(dx, dy, y, d);
    return sqrt(d[0] * d[0] + d[1] * d[1]);
}

}  // namespace

bool net_rows(const int64_t* tree, const double* coord, int64_t n_links, int64_t n_points, bool geographic, NetRows& out, std::string& err) {
    out = NetRows();
    out.real.reserve(size_t(n_links) * NET_REALS);
    out.first.push_back(0);
    for (int64_t l = 0; l < n_links; l++) {
        const int64_t i1 = tree[l * 9 + 1], i2 = tree[l * 9 + 2];
        if (i1 < 0 || i2 < i1 || i2 >= n_points) { err = "link row " + std::to_string(l) + ": its coord rows " + std::to_string(i1) + " .. " + std::to_string(i2) + " are not in coord"; return false; }
        const int64_t np = i2 - i1 + 1;
        const double* c = coord + i1 * 5;   // x, y, distance to the outlet, elevation, contributing area
        auto lengthd = [&](int64_t j) { return float(c[j * 5 + 2]); };
        auto elev = [&](int64_t j) { return float(c[j * 5 + 3]); };
        auto area = [&](int64_t j) { return float(c[j * 5 + 4]); };
        const double x1 = c[0], y1 = c[1];
        double x = x1, y = y1, length = 0., xlast = x1, ylast = y1;
        const double usarea = area(0);
        double dslast = usarea, dsarea = usarea;
        for (int64_t j = 0; j < np; j++) {
            x = c[j * 5];
            y = c[j * 5 + 1];
            const double dl = step_length(x - xlast, y - ylast, y, geographic);
            if (dl > 0.) {
                length = length + dl;
                xlast = x; ylast = y;
                dsarea = dslast;   // the area one moving point back
                dslast = area(j);
            }
        }
        const double drop = elev(0) - elev(np - 1);   // a float difference
        const float dsdist = lengthd(np - 1), usdist = lengthd(0);
        const float middist = (dsdist + usdist) * 0.5;
        const double slope = length > 0. ? drop / length : 0.;
        const double glength = step_length(x - x1, y - y1, y, geographic);
        const double r[NET_REALS] = {length, dsarea, drop, slope, glength, usarea, dsdist, usdist, middist};
        out.real.insert(out.real.end(), r, r + NET_REALS);
        for (int64_t j = np - 1; j >= 0; j--) { out.x.push_back(c[j * 5]); out.y.push_back(c[j * 5 + 1]); }   // np vertices: a link of one point is a line of one vertex
        out.first.push_back(int64_t(out.x.size()));
    }
    return true;
}

void net_layer(const int64_t* tree, int64_t n_links, const NetRows& rows, tdx::LineLayer& L) {
    using tdx::FieldType;
    L = tdx::LineLayer();
    // name, tree column or (negative) -1 - real column; width, decimals (src/streamnet.cpp:163-239).  WSNO is the link number again (:347).
    struct F { const char* name; int col; int width, decimals; };
    static const F fields[17] = {{"LINKNO", 0, 6, 0},     {"DSLINKNO", 3, 6, 0},    {"USLINKNO1", 4, 6, 0},  {"USLINKNO2", 5, 6, 0},   {"DSNODEID", 7, 12, 0},  {"strmOrder", 6, 6, 0},
                                 {"Length", -1, 16, 1},   {"Magnitude", 8, 6, 0},   {"DSContArea", -2, 16, 1}, {"strmDrop", -3, 16, 2}, {"Slope", -4, 16, 12},   {"StraightL", -5, 16, 1},
                                 {"USContArea", -6, 16, 1}, {"WSNO", 0, 6, 0},      {"DOUTEND", -7, 16, 1},  {"DOUTSTART", -8, 16, 1}, {"DOUTMID", -9, 16, 1}};
    for (const F& f : fields) L.add_field(f.name, f.col >= 0 ? FieldType::Integer : FieldType::Real, f.width, f.decimals);
    L.resize(size_t(n_links));
    for (int64_t l = 0; l < n_links; l++) {
        for (size_t k = 0; k < 17; k++) {
            const F& f = fields[k];
            if (f.col >= 0) L.set(size_t(l), k, (long long)int(tree[l * 9 + f.col]));   // (int)cnet[.]
            else L.set(size_t(l), k, rows.real[size_t(l) * NET_REALS + size_t(-f.col - 1)]);
        }
        L.x[size_t(l)].assign(rows.x.begin() + rows.first[size_t(l)], rows.x.begin() + rows.first[size_t(l) + 1]);
        L.y[size_t(l)].assign(rows.y.begin() + rows.first[size_t(l)], rows.y.begin() + rows.first[size_t(l) + 1]);
    }
}

}  // namespace streamnet
