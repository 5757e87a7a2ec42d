#include "catchoutlets.hpp"

#include <cstdlib>
#include <fstream>
#include <sstream>
#include <unordered_map>

namespace tdx {
namespace {

// OGR_F_GetFieldAsDouble / AsInteger on the text of a .dbf cell or a JSON number: a null is 0
double as_double(const std::string& t) { return strtod(t.c_str(), nullptr); }
int32_t as_int(const std::string& t) { return int32_t(strtod(t.c_str(), nullptr)); }

template <class T>
bool read_numbers(const std::string& path, size_t per_row, std::vector<T>& out, std::string& err) {
    std::ifstream f(path);
    if (!f) { err = "cannot open " + path; return false; }
    std::string tok;
    while (f >> tok) {
        char* end = nullptr;
        const double v = strtod(tok.c_str(), &end);
        if (end == tok.c_str() || *end) { err = "not a number in " + path + ": " + tok; return false; }
        out.push_back(T(v));
    }
    if (out.size() % per_row) { err = path + " does not hold rows of " + std::to_string(per_row) + " numbers"; return false; }
    return true;
}

}  // namespace

bool links_from_layer(const LineLayer& L, std::vector<NetLink>& links, std::string& err) {
    static const char* const names[7] = {"LINKNO", "DSLINKNO", "USLINKNO1", "USLINKNO2", "DOUTEND", "DOUTSTART", "USContArea"};
    int col[7];
    for (int k = 0; k < 7; k++)
        if ((col[k] = L.field_index(names[k])) < 0) { err = std::string("the stream network layer has no field ") + names[k]; return false; }
    links.assign(L.x.size(), NetLink());
    for (size_t i = 0; i < L.x.size(); i++) {
        const std::vector<std::string>& v = L.values[i];
        NetLink& k = links[i];
        k.linkno = as_int(v[size_t(col[0])]); k.dslinkno = as_int(v[size_t(col[1])]); k.uslinkno1 = as_int(v[size_t(col[2])]); k.uslinkno2 = as_int(v[size_t(col[3])]);
        k.doutend = as_double(v[size_t(col[4])]); k.doutstart = as_double(v[size_t(col[5])]); k.uscontarea = as_double(v[size_t(col[6])]);
        if (L.x[i].empty()) {
            if (k.dslinkno < 0 || k.uslinkno1 >= 0 || k.uslinkno2 >= 0) { err = "feature " + std::to_string(i) + " of the stream network layer has no vertex"; return false; }
            continue;
        }
        k.down_x = L.x[i].front(); k.down_y = L.y[i].front();
        k.up_x = L.x[i].back(); k.up_y = L.y[i].back();
    }
    return true;
}

bool links_from_text(const std::string& treefile, const std::string& coordfile, std::vector<NetLink>& links, std::string& err) {
    std::vector<int64_t> tree;
    std::vector<double> coord;
    if (!read_numbers(treefile, 9, tree, err) || !read_numbers(coordfile, 5, coord, err)) return false;
    const int64_t n = int64_t(tree.size() / 9), np = int64_t(coord.size() / 5);
    links.assign(size_t(n), NetLink());
    for (int64_t l = 0; l < n; l++) {
        const int64_t* t = &tree[size_t(l) * 9];
        if (t[1] < 0 || t[2] < t[1] || t[2] >= np) { err = "link row " + std::to_string(l) + " of " + treefile + " points outside " + coordfile; return false; }
        const double *first = &coord[size_t(t[1]) * 5], *last = &coord[size_t(t[2]) * 5];
        NetLink& k = links[size_t(l)];
        k.linkno = int32_t(t[0]); k.dslinkno = int32_t(t[3]); k.uslinkno1 = int32_t(t[4]); k.uslinkno2 = int32_t(t[5]);
        k.doutend = last[2]; k.doutstart = first[2]; k.uscontarea = first[4];
        k.down_x = last[0]; k.down_y = last[1]; k.up_x = first[0]; k.up_y = first[1];
    }
    return true;
}

bool catch_outlets(const std::vector<NetLink>& links, const FlowGrid& g, double mindist, int32_t gwstartno, double minarea, std::vector<CatchOutlet>& out,
                   std::string& err) {
    static const int d1[9] = {-99, 0, -1, -1, -1, 0, 1, 1, 1}, d2[9] = {-99, 1, 1, 0, -1, -1, -1, 0, 1};   // row and column steps
    out.clear();
    // the links the reference keeps, in layer order; a link number leads to the FIRST kept link that carries it (its linear search)
    std::vector<int64_t> kept;
    std::unordered_map<int32_t, size_t> at;
    for (size_t i = 0; i < links.size(); i++) {
        const NetLink& k = links[i];
        if (k.dslinkno < 0 || k.uslinkno1 >= 0 || k.uslinkno2 >= 0) { at.emplace(k.linkno, kept.size()); kept.push_back(int64_t(i)); }
    }
    // what a kept link shows as DOUTEND and where its point lies: the downstream end of an outlet link, the upstream end of every other
    auto shown = [&](const NetLink& k) { return k.dslinkno < 0 ? k.doutend : k.doutstart; };
    int32_t gwcount = gwstartno;
    std::vector<char> on_path(kept.size(), 0);
    struct Visit { int32_t link; double downout; int64_t leave; };   // leave >= 0: the walk is done with that kept link
    std::vector<Visit> stack;
    for (size_t s = 0; s < kept.size(); s++) {
        const NetLink& k = links[size_t(kept[s])];
        if (k.dslinkno >= 0) continue;
        const int gx = int((k.down_x - g.xleftedge) / g.dlon), gy = int((g.ytopedge - k.down_y) / g.dlat);   // tiffIO::geoToGlobalXY
        if (gx < 0 || gx >= g.nx || gy < 0 || gy >= g.ny) continue;
        int16_t dirn = 0;
        if (!g.p_at(gx, gy, dirn)) { err = "cannot read the flow direction at column " + std::to_string(gx) + ", row " + std::to_string(gy); return false; }
        if (dirn < 1 || dirn > 8) continue;
        int64_t nextx = gx + d2[dirn], nexty = gy + d1[dirn];
        if (nextx < 0 || nextx >= g.nx || nexty < 0 || nexty >= g.ny) { nextx = gx; nexty = gy; }
        out.push_back({kept[s], g.xleftedge + g.dlon / 2. + double(nextx) * g.dlon, g.ytopedge - g.dlat / 2. - double(nexty) * g.dlat, shown(k), gwcount});   // globalXYToGeo
        gwcount = gwcount + 1;
        // CheckPoint(us1) and all it calls, then CheckPoint(us2): the later call is pushed first
        on_path[s] = 1;
        stack.push_back({0, 0.0, int64_t(s)});
        if (k.uslinkno2 >= 0) stack.push_back({k.uslinkno2, 0.0, -1});
        if (k.uslinkno1 >= 0) stack.push_back({k.uslinkno1, 0.0, -1});
        while (!stack.empty()) {
            const Visit v = stack.back();
            stack.pop_back();
            if (v.leave >= 0) { on_path[size_t(v.leave)] = 0; continue; }
            const auto it = at.find(v.link);
            if (it == at.end()) continue;   // not among the kept ones: a link without any upstream
            const size_t q = it->second;
            if (on_path[q]) { err = "the upstream links of the stream network close a cycle at link " + std::to_string(v.link); return false; }
            const NetLink& u = links[size_t(kept[q])];
            double downout = v.downout;
            if (shown(u) - downout > mindist && u.uscontarea > minarea) {
                out.push_back({kept[q], u.dslinkno < 0 ? u.down_x : u.up_x, u.dslinkno < 0 ? u.down_y : u.up_y, shown(u), gwcount});
                gwcount = gwcount + 1;
                downout = shown(u);
            }
            if (u.uscontarea > minarea) {
                on_path[q] = 1;
                stack.push_back({0, 0.0, int64_t(q)});
                if (u.uslinkno2 >= 0) stack.push_back({u.uslinkno2, downout, -1});
                if (u.uslinkno1 >= 0) stack.push_back({u.uslinkno1, downout, -1});
            }
        }
    }
    return true;
}

void catch_outlets_layer(const std::vector<NetLink>& links, const std::vector<CatchOutlet>& outlets, PointLayer& L) {
    L = PointLayer();
    for (const char* name : {"LINKNO", "DSLINKNO", "USLINKNO1", "USLINKNO2"}) L.add_field(name, FieldType::Integer, 6);
    L.add_field("DOUTEND", FieldType::Real, 16, 1);
    L.add_field("Id", FieldType::Integer, 10);
    L.resize(outlets.size());
    for (size_t i = 0; i < outlets.size(); i++) {
        const CatchOutlet& o = outlets[i];
        const NetLink& k = links[size_t(o.row)];
        L.x[i] = o.x; L.y[i] = o.y;
        L.set(i, 0, (long long)k.linkno); L.set(i, 1, (long long)k.dslinkno); L.set(i, 2, (long long)k.uslinkno1); L.set(i, 3, (long long)k.uslinkno2);
        L.set(i, 4, o.doutend);
        L.set(i, 5, (long long)o.id);
    }
}

}  // namespace tdx
