#include "vector_layer.hpp"

#include <algorithm>
#include <cctype>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <utility>

namespace tdx {
const char* const kLayerKindsMessage = "supported point layers: ESRI shapefile (.shp) and GeoJSON (.json, .geojson)";
const char* const kLineLayerKindsMessage = "supported line layers: ESRI shapefile (.shp) and GeoJSON (.json, .geojson)";
const char* const kPolygonLayerKindsMessage = "supported polygon layers: ESRI shapefile (.shp) and GeoJSON (.json, .geojson)";

namespace {
std::string lower_ext(const std::string& p) {
    const size_t d = p.rfind('.'), s = p.find_last_of("/\\");
    if (d == std::string::npos || (s != std::string::npos && d < s)) return "";
    std::string e = p.substr(d);
    for (char& c : e) c = char(tolower((unsigned char)c));
    return e;
}
std::string with_ext(const std::string& p, const char* ext) { return p.substr(0, p.rfind('.')) + ext; }
std::string trim(const std::string& s) {
    size_t a = 0, b = s.size();
    while (a < b && (s[a] == ' ' || s[a] == '\0')) a++;
    while (b > a && (s[b - 1] == ' ' || s[b - 1] == '\0')) b--;
    return s.substr(a, b - a);
}
bool slurp(const std::string& path, std::string& out) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    std::stringstream ss; ss << f.rdbuf();
    out = ss.str();
    return true;
}
bool spill(const std::string& path, const std::string& bytes, std::string& err) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) { err = "cannot create " + path; return false; }
    const bool ok = bytes.empty() || fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
    if (fclose(f) != 0 || !ok) { err = "cannot write " + path; return false; }
    return true;
}
void put_be32(std::string& s, uint32_t v) { const char b[4] = {char(v >> 24), char(v >> 16), char(v >> 8), char(v)}; s.append(b, 4); }
void put_le32(std::string& s, uint32_t v) { const char b[4] = {char(v), char(v >> 8), char(v >> 16), char(v >> 24)}; s.append(b, 4); }
void put_le64f(std::string& s, double v) { char b[8]; memcpy(b, &v, 8); s.append(b, 8); }   // the host is little-endian
FieldType type_of_dbf(char t, int decimals) { return (t == 'N' || t == 'F') ? (decimals == 0 ? FieldType::Integer : FieldType::Real) : FieldType::String; }
int default_width(FieldType t) { return t == FieldType::Integer ? 9 : t == FieldType::Real ? 24 : 80; }

// ---- .shp / .shx / .dbf
// xmin, ymin, xmax, ymax of a run of vertices, grown over calls; zeros while no vertex has been seen
struct Box {
    double b[4] = {0, 0, 0, 0};
    bool any = false;
    void add(const std::vector<double>& x, const std::vector<double>& y) {
        for (size_t i = 0; i < x.size(); i++) {
            if (!any) { b[0] = b[2] = x[i]; b[1] = b[3] = y[i]; any = true; continue; }
            b[0] = std::min(b[0], x[i]); b[2] = std::max(b[2], x[i]);
            b[1] = std::min(b[1], y[i]); b[3] = std::max(b[3], y[i]);
        }
    }
};
std::string shape_header(uint32_t words, uint32_t shape_type, const Box& box) {
    std::string h;
    put_be32(h, 9994);
    for (int i = 0; i < 5; i++) put_be32(h, 0);
    put_be32(h, words);
    put_le32(h, 1000);
    put_le32(h, shape_type);
    for (double b : box.b) put_le64f(h, b);
    for (int i = 0; i < 4; i++) put_le64f(h, 0.0);   // z and m ranges
    return h;
}

// the bytes of one value in a .dbf column of `width` characters
std::string dbf_cell(const LayerField& f, int width, int decimals, const std::string& v) {
    if (!f.dbf_descriptor.empty()) return v.size() == size_t(width) ? v : (v + std::string(size_t(width), ' ')).substr(0, size_t(width));
    std::string t = v;
    if (f.type == FieldType::Real && !v.empty()) {
        char buf[400];
        snprintf(buf, sizeof buf, "%*.*f", width, decimals, strtod(v.c_str(), nullptr));
        t = buf;
        if (t.size() > size_t(width)) { snprintf(buf, sizeof buf, "%*.*e", width, std::max(0, width - 8), strtod(v.c_str(), nullptr)); t = buf; }
    }
    if (t.size() > size_t(width)) t.resize(size_t(width));
    const std::string pad(size_t(width) - t.size(), ' ');
    return f.type == FieldType::String ? t + pad : pad + t;
}

// the .dbf of a table of n features
bool dbf_bytes(const LayerTable& L, size_t n, std::string& dbf, std::string& err) {
    // widths: a carried-over column keeps its own; otherwise the field's, or the type's default (an Integer column grows to its longest value)
    std::vector<int> width(L.fields.size()), decimals(L.fields.size());
    size_t reclen = 1;
    for (size_t k = 0; k < L.fields.size(); k++) {
        const LayerField& f = L.fields[k];
        if (!f.dbf_descriptor.empty()) { width[k] = (unsigned char)f.dbf_descriptor[16]; decimals[k] = (unsigned char)f.dbf_descriptor[17]; }
        else {
            width[k] = f.width > 0 ? f.width : default_width(f.type);
            decimals[k] = f.type == FieldType::Real ? (f.width > 0 ? f.decimals : 15) : 0;
            if (f.type == FieldType::Integer)
                for (size_t i = 0; i < n; i++) width[k] = std::max(width[k], int(L.values[i][k].size()));
            width[k] = std::min(width[k], 254);
        }
        reclen += size_t(width[k]);
    }
    if (reclen > 65535 || L.fields.size() > 2046) { err = "too many fields for a .dbf"; return false; }
    const char date[4] = {0x03, 95, 7, 26};   // version, and a fixed date: the same layer gives the same bytes
    dbf.append(date, 4);
    put_le32(dbf, uint32_t(n));
    const uint16_t hlen = uint16_t(32 + 32 * L.fields.size() + 1), rlen = uint16_t(reclen);
    dbf.push_back(char(hlen & 255)); dbf.push_back(char(hlen >> 8)); dbf.push_back(char(rlen & 255)); dbf.push_back(char(rlen >> 8));
    dbf.append(20, '\0');
    for (size_t k = 0; k < L.fields.size(); k++) {
        const LayerField& f = L.fields[k];
        if (!f.dbf_descriptor.empty()) { dbf += f.dbf_descriptor; continue; }
        std::string d(32, '\0');
        memcpy(&d[0], f.name.data(), std::min<size_t>(f.name.size(), 10));
        d[11] = f.type == FieldType::String ? 'C' : 'N';
        d[16] = char(width[k]); d[17] = char(decimals[k]);
        dbf += d;
    }
    dbf.push_back('\r');
    for (size_t i = 0; i < n; i++) {
        dbf.push_back(' ');
        for (size_t k = 0; k < L.fields.size(); k++) dbf += dbf_cell(L.fields[k], width[k], decimals[k], L.values[i][k]);
    }
    dbf.push_back('\x1a');
    return true;
}

bool write_shapefile(const std::string& path, const PointLayer& L, std::string& err) {
    const size_t n = L.x.size();
    if (n > 0x7000000u) { err = "too many points for a shapefile"; return false; }
    Box box;
    box.add(L.x, L.y);
    std::string shp = shape_header(uint32_t(50 + 14 * n), 1, box), shx = shape_header(uint32_t(50 + 4 * n), 1, box), dbf;
    for (size_t i = 0; i < n; i++) {
        put_be32(shx, uint32_t(50 + 14 * i)); put_be32(shx, 10);
        put_be32(shp, uint32_t(i + 1)); put_be32(shp, 10);
        put_le32(shp, 1); put_le64f(shp, L.x[i]); put_le64f(shp, L.y[i]);
    }
    return dbf_bytes(L, n, dbf, err) && spill(path, shp, err) && spill(with_ext(path, ".shx"), shx, err) && spill(with_ext(path, ".dbf"), dbf, err);
}

// PolyLine records: shape type, box, one part that starts at vertex 0, the vertices - 24 + 8 * vertices 16-bit words each
bool write_line_shapefile(const std::string& path, const LineLayer& L, std::string& err) {
    const size_t n = L.x.size();
    size_t words = 50;
    Box all;
    for (size_t i = 0; i < n; i++) { words += 4 + 24 + 8 * L.x[i].size(); all.add(L.x[i], L.y[i]); }
    if (n > 0x7000000u || words > 0x7fffffffu) { err = "too many vertices for a shapefile"; return false; }
    std::string shp = shape_header(uint32_t(words), 3, all), shx = shape_header(uint32_t(50 + 4 * n), 3, all), dbf;
    size_t at = 50;
    for (size_t i = 0; i < n; i++) {
        const size_t np = L.x[i].size(), len = 24 + 8 * np;
        put_be32(shx, uint32_t(at)); put_be32(shx, uint32_t(len));
        put_be32(shp, uint32_t(i + 1)); put_be32(shp, uint32_t(len));
        put_le32(shp, 3);
        Box b;
        b.add(L.x[i], L.y[i]);
        for (double v : b.b) put_le64f(shp, v);
        put_le32(shp, 1); put_le32(shp, uint32_t(np)); put_le32(shp, 0);
        for (size_t k = 0; k < np; k++) { put_le64f(shp, L.x[i][k]); put_le64f(shp, L.y[i][k]); }
        at += 4 + len;
    }
    return dbf_bytes(L, n, dbf, err) && spill(path, shp, err) && spill(with_ext(path, ".shx"), shx, err) && spill(with_ext(path, ".dbf"), dbf, err);
}

// Polygon records: shape type, box, the part and point counts, the first point of every part (ring), the points - 22 + 2 * parts + 8 * points 16-bit words each
bool write_polygon_shapefile(const std::string& path, const PolygonLayer& L, std::string& err) {
    const size_t n = L.polygons.size();
    size_t words = 50;
    Box all;
    std::vector<size_t> nparts(n, 0), npoints(n, 0);
    for (size_t i = 0; i < n; i++) {
        for (const PolygonLayer::Polygon& pg : L.polygons[i])
            for (const PolygonLayer::Ring& rg : pg) { nparts[i]++; npoints[i] += rg.x.size(); all.add(rg.x, rg.y); }
        if (npoints[i] > 0x7000000u) { err = "too many vertices for a shapefile"; return false; }
        words += 4 + 22 + 2 * nparts[i] + 8 * npoints[i];
    }
    if (n > 0x7000000u || words > 0x7fffffffu) { err = "too many vertices for a shapefile"; return false; }
    std::string shp = shape_header(uint32_t(words), 5, all), shx = shape_header(uint32_t(50 + 4 * n), 5, all), dbf;
    shp.reserve(words * 2);
    size_t at = 50;
    for (size_t i = 0; i < n; i++) {
        const size_t len = 22 + 2 * nparts[i] + 8 * npoints[i];
        put_be32(shx, uint32_t(at)); put_be32(shx, uint32_t(len));
        put_be32(shp, uint32_t(i + 1)); put_be32(shp, uint32_t(len));
        put_le32(shp, 5);
        Box b;
        for (const PolygonLayer::Polygon& pg : L.polygons[i])
            for (const PolygonLayer::Ring& rg : pg) b.add(rg.x, rg.y);
        for (double v : b.b) put_le64f(shp, v);
        put_le32(shp, uint32_t(nparts[i])); put_le32(shp, uint32_t(npoints[i]));
        size_t first = 0;
        for (const PolygonLayer::Polygon& pg : L.polygons[i])
            for (const PolygonLayer::Ring& rg : pg) { put_le32(shp, uint32_t(first)); first += rg.x.size(); }
        for (const PolygonLayer::Polygon& pg : L.polygons[i])
            for (const PolygonLayer::Ring& rg : pg)
                for (size_t k = 0; k < rg.x.size(); k++) { put_le64f(shp, rg.x[k]); put_le64f(shp, rg.y[k]); }
        at += 4 + len;
    }
    return dbf_bytes(L, n, dbf, err) && spill(path, shp, err) && spill(with_ext(path, ".shx"), shx, err) && spill(with_ext(path, ".dbf"), dbf, err);
}

uint32_t rd_be32(const unsigned char* q) { return (uint32_t(q[0]) << 24) | (uint32_t(q[1]) << 16) | (uint32_t(q[2]) << 8) | q[3]; }
uint32_t rd_le32(const unsigned char* q) { return uint32_t(q[0]) | (uint32_t(q[1]) << 8) | (uint32_t(q[2]) << 16) | (uint32_t(q[3]) << 24); }
double rd_le64f(const unsigned char* q) { double v; memcpy(&v, q, 8); return v; }

// The records of a .shp of type PolyLine, PolyLineZ or PolyLineM: every record is a feature (a null shape, or one of another type, without vertices, so
// that the rows of the .dbf stay with their records); every count is checked against the record's length before a vertex is read
bool read_line_shapes(const std::string& path, LineLayer& L, std::string& err) {
    std::string bytes;
    if (!slurp(path, bytes)) { err = "cannot open " + path; return false; }
    const unsigned char* u = reinterpret_cast<const unsigned char*>(bytes.data());
    if (bytes.size() < 100 || rd_be32(u) != 9994) { err = "not a shapefile: " + path; return false; }
    const uint32_t type = rd_le32(u + 32);
    if (!(type == 3 || type == 13 || type == 23)) { err = "shapefile layer is not a line layer: " + path; return false; }
    size_t pos = 100;
    while (pos + 8 <= bytes.size()) {
        const size_t clen = size_t(rd_be32(u + pos + 4)) * 2;
        pos += 8;
        if (clen > bytes.size() - pos) { err = "truncated record in " + path; return false; }
        std::vector<double> x, y;
        const uint32_t t = clen >= 4 ? rd_le32(u + pos) : 0;
        if (t == 3 || t == 13 || t == 23) {
            if (clen < 44) { err = "short line record in " + path; return false; }
            const size_t nparts = rd_le32(u + pos + 36), npoints = rd_le32(u + pos + 40);
            if (nparts > clen / 4 || npoints > clen / 16 || 44 + 4 * nparts + 16 * npoints > clen) { err = "line record with impossible counts in " + path; return false; }
            size_t first = 0, last = npoints;
            if (nparts >= 1) first = rd_le32(u + pos + 44);
            if (nparts >= 2) last = rd_le32(u + pos + 48);
            if (first > last || last > npoints) { err = "line record with impossible parts in " + path; return false; }
            const unsigned char* pts = u + pos + 44 + 4 * nparts;
            for (size_t k = first; k < last; k++) { x.push_back(rd_le64f(pts + 16 * k)); y.push_back(rd_le64f(pts + 16 * k + 8)); }
        }
        L.x.push_back(std::move(x)); L.y.push_back(std::move(y));
        pos += clen;
    }
    return true;
}

// The records of a .shp of type Polygon, PolygonZ or PolygonM: every record is a feature (a null shape, or one of another type, without rings, so that
// the rows of the .dbf stay with their records); every part is a ring of a polygon of its own.  Record lengths, counts and part indices are checked
// against what was read before a vertex is taken; Z and M, which follow the points, are not looked at
bool read_polygon_shapes(const std::string& path, PolygonLayer& L, std::string& err) {
    std::string bytes;
    if (!slurp(path, bytes)) { err = "cannot open " + path; return false; }
    const unsigned char* u = reinterpret_cast<const unsigned char*>(bytes.data());
    if (bytes.size() < 100 || rd_be32(u) != 9994) { err = "not a shapefile: " + path; return false; }
    const uint32_t type = rd_le32(u + 32);
    if (!(type == 5 || type == 15 || type == 25)) { err = "shapefile layer is not a polygon layer: " + path; return false; }
    size_t pos = 100;
    while (pos < bytes.size()) {
        if (bytes.size() - pos < 8) { err = "truncated record header in " + path; return false; }
        const size_t clen = size_t(rd_be32(u + pos + 4)) * 2;
        pos += 8;
        if (clen > bytes.size() - pos) { err = "truncated record in " + path; return false; }
        std::vector<PolygonLayer::Polygon> polys;
        const uint32_t t = clen >= 4 ? rd_le32(u + pos) : 0;
        if (t == 5 || t == 15 || t == 25) {
            if (clen < 44) { err = "short polygon record in " + path; return false; }
            const size_t nparts = rd_le32(u + pos + 36), npoints = rd_le32(u + pos + 40);
            if (nparts > clen / 4 || npoints > clen / 16 || 44 + 4 * nparts + 16 * npoints > clen) { err = "polygon record with impossible counts in " + path; return false; }
            const unsigned char* parts = u + pos + 44;
            const unsigned char* pts = parts + 4 * nparts;
            for (size_t q = 0; q < nparts; q++) {
                const size_t first = rd_le32(parts + 4 * q), last = q + 1 < nparts ? size_t(rd_le32(parts + 4 * (q + 1))) : npoints;
                if (first > last || last > npoints) { err = "polygon record with impossible parts in " + path; return false; }
                PolygonLayer::Ring rg;
                for (size_t k = first; k < last; k++) { rg.x.push_back(rd_le64f(pts + 16 * k)); rg.y.push_back(rd_le64f(pts + 16 * k + 8)); }
                polys.push_back(PolygonLayer::Polygon{std::move(rg)});
            }
        }
        L.polygons.push_back(std::move(polys));
        pos += clen;
    }
    return true;
}

bool read_dbf_fields(const std::string& shp_path, size_t n_features, LayerTable& L, std::string& err) {
    std::string b;
    if (!slurp(with_ext(shp_path, ".dbf"), b) && !slurp(with_ext(shp_path, ".DBF"), b)) return true;   // a .shp without attributes: no field
    if (b.size() < 33) { err = "not a .dbf file next to " + shp_path; return false; }
    const unsigned char* u = reinterpret_cast<const unsigned char*>(b.data());
    const size_t nrec = size_t(u[4]) | size_t(u[5]) << 8 | size_t(u[6]) << 16 | size_t(u[7]) << 24, hlen = size_t(u[8]) | size_t(u[9]) << 8,
                 rlen = size_t(u[10]) | size_t(u[11]) << 8;
    std::vector<size_t> off;
    size_t o = 1;
    for (size_t q = 32; q + 32 <= hlen && q + 32 <= b.size() && u[q] != 0x0d; q += 32) {
        LayerField f;
        f.dbf_descriptor = b.substr(q, 32);
        f.name = std::string(f.dbf_descriptor.c_str(), strnlen(f.dbf_descriptor.c_str(), 11));
        f.width = u[q + 16]; f.decimals = u[q + 17];
        f.type = type_of_dbf(char(u[q + 11]), f.decimals);
        L.fields.push_back(f);
        off.push_back(o);
        o += size_t(f.width);
    }
    if (o > rlen || nrec != n_features || hlen + nrec * rlen > b.size()) { err = "the .dbf next to " + shp_path + " does not match its features"; return false; }
    for (size_t i = 0; i < nrec; i++)
        for (size_t k = 0; k < L.fields.size(); k++) L.values[i].push_back(b.substr(hlen + i * rlen + off[k], size_t(L.fields[k].width)));
    return true;
}

// ---- GeoJSON
struct JVal {
    enum Kind { Null, Bool, Number, String, Array, Object } kind = Null;
    std::string text;   // Number: as written; String: decoded; Bool: "true" / "false"
    std::vector<JVal> arr;
    std::vector<std::pair<std::string, JVal>> obj;
    const JVal* get(const char* key) const {
        for (const auto& kv : obj) if (kv.first == key) return &kv.second;
        return nullptr;
    }
};
struct JParser {
    const std::string& s;
    size_t p = 0;
    bool ok = true;
    int depth = 0;
    explicit JParser(const std::string& text) : s(text) {}
    void ws() { while (p < s.size() && isspace((unsigned char)s[p])) p++; }
    void utf8(std::string& out, unsigned c) {
        if (c < 0x80) out.push_back(char(c));
        else if (c < 0x800) { out.push_back(char(0xc0 | (c >> 6))); out.push_back(char(0x80 | (c & 63))); }
        else { out.push_back(char(0xe0 | (c >> 12))); out.push_back(char(0x80 | ((c >> 6) & 63))); out.push_back(char(0x80 | (c & 63))); }
    }
    std::string str() {
        std::string out;
        p++;   // the opening quote
        while (p < s.size() && s[p] != '"') {
            if (s[p] != '\\') { out.push_back(s[p++]); continue; }
            if (++p >= s.size()) break;
            const char c = s[p++];
            switch (c) {
            case 'n': out.push_back('\n'); break;
            case 't': out.push_back('\t'); break;
            case 'r': out.push_back('\r'); break;
            case 'b': out.push_back('\b'); break;
            case 'f': out.push_back('\f'); break;
            case 'u': {
                unsigned v = 0;
                for (int i = 0; i < 4 && p < s.size(); i++, p++) v = v * 16 + unsigned(isdigit((unsigned char)s[p]) ? s[p] - '0' : (tolower((unsigned char)s[p]) - 'a' + 10) & 15);
                utf8(out, v);
                break;
            }
            default: out.push_back(c);
            }
        }
        if (p >= s.size()) ok = false; else p++;
        return out;
    }
    JVal value() {
        JVal v;
        ws();
        if (p >= s.size() || ++depth > 200) { ok = false; return v; }
        const char c = s[p];
        if (c == '{') {
            v.kind = JVal::Object; p++; ws();
            if (p < s.size() && s[p] == '}') p++;
            else
                while (ok) {
                    ws();
                    if (p >= s.size() || s[p] != '"') { ok = false; break; }
                    std::string k = str();
                    ws();
                    if (p >= s.size() || s[p] != ':') { ok = false; break; }
                    p++;
                    JVal e = value();
                    v.obj.emplace_back(std::move(k), std::move(e));
                    ws();
                    if (p < s.size() && s[p] == ',') { p++; continue; }
                    if (p < s.size() && s[p] == '}') { p++; break; }
                    ok = false;
                }
        } else if (c == '[') {
            v.kind = JVal::Array; p++; ws();
            if (p < s.size() && s[p] == ']') p++;
            else
                while (ok) {
                    v.arr.push_back(value());
                    ws();
                    if (p < s.size() && s[p] == ',') { p++; continue; }
                    if (p < s.size() && s[p] == ']') { p++; break; }
                    ok = false;
                }
        } else if (c == '"') { v.kind = JVal::String; v.text = str(); }
        else if (s.compare(p, 4, "true") == 0) { v.kind = JVal::Bool; v.text = "true"; p += 4; }
        else if (s.compare(p, 5, "false") == 0) { v.kind = JVal::Bool; v.text = "false"; p += 5; }
        else if (s.compare(p, 4, "null") == 0) { p += 4; }
        else {
            const size_t a = p;
            while (p < s.size() && (isdigit((unsigned char)s[p]) || s[p] == '-' || s[p] == '+' || s[p] == '.' || s[p] == 'e' || s[p] == 'E')) p++;
            if (p == a) ok = false;
            v.kind = JVal::Number; v.text = s.substr(a, p - a);
        }
        depth--;
        return v;
    }
};
void collect_point_features(const JVal& v, std::vector<const JVal*>& out) {   // in document order, the features read_outlets() sees: flat [x, y] coordinates
    if (v.kind == JVal::Object) {
        const JVal* g = v.get("geometry");
        const JVal* c = g && g->kind == JVal::Object ? g->get("coordinates") : nullptr;
        if (c) { if (c->kind == JVal::Array && c->arr.size() >= 2 && c->arr[0].kind == JVal::Number) out.push_back(&v); return; }
        for (const auto& kv : v.obj) collect_point_features(kv.second, out);
    } else if (v.kind == JVal::Array)
        for (const JVal& e : v.arr) collect_point_features(e, out);
}
bool is_int_text(const std::string& t) {
    if (t.find_first_of(".eE") != std::string::npos) return false;
    const long long v = strtoll(t.c_str(), nullptr, 10);
    return v >= INT_MIN && v <= INT_MAX;
}
// the properties of features -> fields (in order of first appearance; Integer until a value says otherwise) and values
void fill_properties(const std::vector<const JVal*>& feats, LayerTable& L) {
    for (size_t i = 0; i < feats.size(); i++) {
        const JVal* pr = feats[i]->get("properties");
        if (!pr || pr->kind != JVal::Object) continue;
        for (const auto& kv : pr->obj) {
            size_t k = 0;
            while (k < L.fields.size() && L.fields[k].name != kv.first) k++;
            if (k == L.fields.size()) L.add_field(kv.first, FieldType::Integer);
            const JVal& e = kv.second;
            if (e.kind == JVal::Null) continue;
            LayerField& f = L.fields[k];
            if (e.kind != JVal::Number) f.type = FieldType::String;
            else if (!is_int_text(e.text) && f.type == FieldType::Integer) f.type = FieldType::Real;
            L.values[i][k] = (e.kind == JVal::Array || e.kind == JVal::Object) ? std::string("(nested)") : e.text;
        }
    }
}
bool read_geojson_fields(const std::string& path, size_t n_features, PointLayer& L, std::string& err) {
    std::string text;
    if (!slurp(path, text)) { err = "cannot open " + path; return false; }
    JParser jp(text);
    const JVal root = jp.value();
    if (!jp.ok) { err = "cannot parse " + path; return false; }
    std::vector<const JVal*> feats;
    collect_point_features(root, feats);
    if (feats.size() != n_features) { err = "the properties of " + path + " do not match its points"; return false; }
    fill_properties(feats, L);
    return true;
}

std::string json_string(const std::string& s) {
    std::string o = "\"";
    for (unsigned char c : s) {
        if (c == '"' || c == '\\') { o.push_back('\\'); o.push_back(char(c)); }
        else if (c < 0x20) { char b[8]; snprintf(b, sizeof b, "\\u%04x", c); o += b; }
        else o.push_back(char(c));
    }
    return o + "\"";
}
std::string json_number(const std::string& t, bool integer) {
    char* end = nullptr;
    if (integer) {
        const long long v = strtoll(t.c_str(), &end, 10);
        if (end == t.c_str()) return "null";
        return std::to_string(v);
    }
    const double v = strtod(t.c_str(), &end);
    if (end == t.c_str() || !std::isfinite(v)) return "null";
    char b[64];
    snprintf(b, sizeof b, "%.17g", v);
    std::string s = b;
    if (s.find_first_of(".e") == std::string::npos) s += ".0";   // a Real stays one for its reader: 3.0, and -0.0 keeps its sign
    return s;
}
// the head of feature i up to its geometry
std::string feature_head(const LayerTable& L, size_t i) {
    std::string o = "{ \"type\": \"Feature\", \"properties\": { ";
    for (size_t k = 0; k < L.fields.size(); k++) {
        const std::string v = trim(L.values[i][k]);
        o += (k ? ", " : "") + json_string(L.fields[k].name) + ": ";
        o += v.empty() ? "null" : L.fields[k].type == FieldType::String ? json_string(v) : json_number(v, L.fields[k].type == FieldType::Integer);
    }
    return o + " }, \"geometry\": { \"type\": ";
}
std::string position(double x, double y) {
    char c[96];
    snprintf(c, sizeof c, "[ %.17g, %.17g ]", x, y);
    return c;
}
bool write_geojson(const std::string& path, const PointLayer& L, std::string& err) {
    std::string o = "{\n\"type\": \"FeatureCollection\",\n\"features\": [\n";
    for (size_t i = 0; i < L.x.size(); i++)
        o += feature_head(L, i) + "\"Point\", \"coordinates\": " + position(L.x[i], L.y[i]) + " } }" + (i + 1 < L.x.size() ? ",\n" : "\n");
    o += "]\n}\n";
    return spill(path, o, err);
}
bool write_line_geojson(const std::string& path, const LineLayer& L, std::string& err) {
    std::string o = "{\n\"type\": \"FeatureCollection\",\n\"features\": [\n";
    for (size_t i = 0; i < L.x.size(); i++) {
        o += feature_head(L, i) + "\"LineString\", \"coordinates\": [ ";
        for (size_t k = 0; k < L.x[i].size(); k++) o += (k ? ", " : "") + position(L.x[i][k], L.y[i][k]);
        o += std::string(" ] } }") + (i + 1 < L.x.size() ? ",\n" : "\n");
    }
    o += "]\n}\n";
    return spill(path, o, err);
}

// the rings of one polygon, each reversed (RFC 7946)
void polygon_json(std::string& o, const PolygonLayer::Polygon& pg) {
    o += "[ ";
    for (size_t q = 0; q < pg.size(); q++) {
        o += q ? ", [ " : "[ ";
        for (size_t k = pg[q].x.size(); k-- > 0;) { o += position(pg[q].x[k], pg[q].y[k]); if (k) o += ", "; }
        o += " ]";
    }
    o += " ]";
}
bool write_polygon_geojson(const std::string& path, const PolygonLayer& L, std::string& err) {
    std::string o = "{\n\"type\": \"FeatureCollection\",\n\"features\": [\n";
    const size_t n = L.polygons.size();
    for (size_t i = 0; i < n; i++) {
        const std::vector<PolygonLayer::Polygon>& f = L.polygons[i];
        o += feature_head(L, i);
        if (f.size() == 1) { o += "\"Polygon\", \"coordinates\": "; polygon_json(o, f[0]); }
        else {
            o += "\"MultiPolygon\", \"coordinates\": [ ";
            for (size_t p = 0; p < f.size(); p++) { if (p) o += ", "; polygon_json(o, f[p]); }
            o += " ]";
        }
        o += std::string(" } }") + (i + 1 < n ? ",\n" : "\n");
    }
    o += "]\n}\n";
    return spill(path, o, err);
}

// in document order, the features whose geometry is a LineString (or a MultiLineString: its first part)
void collect_line_features(const JVal& v, std::vector<const JVal*>& feats, std::vector<const JVal*>& coords) {
    if (v.kind == JVal::Object) {
        const JVal* g = v.get("geometry");
        if (g && g->kind == JVal::Object) {
            const JVal* t = g->get("type");
            const JVal* c = g->get("coordinates");
            if (t && c && c->kind == JVal::Array) {
                if (t->text == "LineString") { feats.push_back(&v); coords.push_back(c); }
                else if (t->text == "MultiLineString" && !c->arr.empty() && c->arr[0].kind == JVal::Array) { feats.push_back(&v); coords.push_back(&c->arr[0]); }
            }
            return;
        }
        for (const auto& kv : v.obj) collect_line_features(kv.second, feats, coords);
    } else if (v.kind == JVal::Array)
        for (const JVal& e : v.arr) collect_line_features(e, feats, coords);
}
bool read_line_geojson(const std::string& path, LineLayer& L, std::string& err) {
    std::string text;
    if (!slurp(path, text)) { err = "cannot open " + path; return false; }
    JParser jp(text);
    const JVal root = jp.value();
    if (!jp.ok) { err = "cannot parse " + path; return false; }
    std::vector<const JVal*> feats, coords;
    collect_line_features(root, feats, coords);
    L.resize(feats.size());
    for (size_t i = 0; i < feats.size(); i++)
        for (const JVal& pt : coords[i]->arr) {
            if (pt.kind != JVal::Array || pt.arr.size() < 2 || pt.arr[0].kind != JVal::Number || pt.arr[1].kind != JVal::Number) { err = "a position of " + path + " is not [x, y]"; return false; }
            L.x[i].push_back(strtod(pt.arr[0].text.c_str(), nullptr));
            L.y[i].push_back(strtod(pt.arr[1].text.c_str(), nullptr));
        }
    fill_properties(feats, L);
    return true;
}

// in document order, the features whose geometry is a Polygon or a MultiPolygon
void collect_polygon_features(const JVal& v, std::vector<const JVal*>& feats) {
    if (v.kind == JVal::Object) {
        const JVal* g = v.get("geometry");
        if (g && g->kind == JVal::Object) {
            const JVal* t = g->get("type");
            const JVal* c = g->get("coordinates");
            if (t && c && c->kind == JVal::Array && (t->text == "Polygon" || t->text == "MultiPolygon")) feats.push_back(&v);
            return;
        }
        for (const auto& kv : v.obj) collect_polygon_features(kv.second, feats);
    } else if (v.kind == JVal::Array)
        for (const JVal& e : v.arr) collect_polygon_features(e, feats);
}
bool number_of(const JVal& v, double& out) {   // a JSON number all of whose text is one
    if (v.kind != JVal::Number || v.text.empty()) return false;
    char* end = nullptr;
    out = strtod(v.text.c_str(), &end);
    return end == v.text.c_str() + v.text.size();
}
bool ring_of(const JVal& r, PolygonLayer::Ring& rg) {
    if (r.kind != JVal::Array) return false;
    for (const JVal& pt : r.arr) {
        double x, y;
        if (pt.kind != JVal::Array || pt.arr.size() < 2 || !number_of(pt.arr[0], x) || !number_of(pt.arr[1], y)) return false;
        rg.x.push_back(x); rg.y.push_back(y);
    }
    return true;
}
bool read_polygon_geojson(const std::string& path, PolygonLayer& L, std::string& err) {
    std::string text;
    if (!slurp(path, text)) { err = "cannot open " + path; return false; }
    JParser jp(text);
    const JVal root = jp.value();
    jp.ws();
    if (!jp.ok || jp.p != text.size()) { err = "cannot parse " + path; return false; }
    std::vector<const JVal*> feats;
    collect_polygon_features(root, feats);
    L.resize(feats.size());
    for (size_t i = 0; i < feats.size(); i++) {
        const JVal* g = feats[i]->get("geometry");
        const JVal* c = g->get("coordinates");
        const bool multi = g->get("type")->text == "MultiPolygon";
        for (const JVal& a : c->arr) {
            if (multi && a.kind != JVal::Array) { err = "a polygon of " + path + " is not a list of rings"; return false; }
            const std::vector<JVal>& rings = multi ? a.arr : c->arr;
            for (const JVal& r : rings) {
                PolygonLayer::Ring rg;
                if (!ring_of(r, rg)) { err = "a position of " + path + " is not [x, y]"; return false; }
                L.polygons[i].push_back(PolygonLayer::Polygon{std::move(rg)});
            }
            if (!multi) break;
        }
    }
    fill_properties(feats, L);
    return true;
}

bool read_text_fields(const std::string& path, size_t n_features, PointLayer& L, std::string& err) {
    std::ifstream f(path);
    if (!f) { err = "cannot open " + path; return false; }
    const size_t k = L.add_field("id", FieldType::Integer);
    std::string line;
    size_t i = 0;
    while (std::getline(f, line)) {   // the lines read_outlets() takes (outlets.cpp: read_text)
        const size_t h = line.find('#');
        if (h != std::string::npos) line.resize(h);
        for (char& c : line) if (c == ',' || c == ';' || c == '\t') c = ' ';
        std::istringstream is(line);
        double vx, vy, vid;
        if (!(is >> vx >> vy)) continue;
        if (i >= n_features) { err = "the ids of " + path + " do not match its points"; return false; }
        L.set(i, k, (long long)((is >> vid) ? int(vid) : int(i) + 1));
        i++;
    }
    if (i != n_features) { err = "the ids of " + path + " do not match its points"; return false; }
    return true;
}
}  // namespace

size_t LayerTable::add_field(const std::string& name, FieldType type, int width, int decimals) {
    LayerField f;
    f.name = name; f.type = type; f.width = width; f.decimals = decimals;
    fields.push_back(f);
    for (auto& row : values) row.resize(fields.size());
    return fields.size() - 1;
}
int LayerTable::field_index(const std::string& name) const {
    for (size_t k = 0; k < fields.size(); k++) if (fields[k].name == name) return int(k);
    return -1;
}
void LayerTable::set(size_t feature, size_t field, long long v) { values[feature][field] = std::to_string(v); }
void LayerTable::set(size_t feature, size_t field, double v) {
    char b[64];
    snprintf(b, sizeof b, "%.17g", v);
    values[feature][field] = b;
}
void PointLayer::resize(size_t n) {
    x.resize(n); y.resize(n);
    values.resize(n);
    for (auto& row : values) row.resize(fields.size());
}
void PolygonLayer::resize(size_t n) {
    polygons.assign(n, {});
    values.resize(n);
    for (auto& row : values) row.resize(fields.size());
}
void LineLayer::resize(size_t n) {
    x.assign(n, {}); y.assign(n, {});
    values.resize(n);
    for (auto& row : values) row.resize(fields.size());
}

LayerKind layer_kind(const std::string& path) {
    const std::string e = lower_ext(path);
    return e == ".shp" ? LayerKind::Shapefile : (e == ".json" || e == ".geojson") ? LayerKind::GeoJSON : LayerKind::None;
}
std::vector<std::string> layer_files(const std::string& path) {
    if (layer_kind(path) == LayerKind::Shapefile) return {path, with_ext(path, ".shx"), with_ext(path, ".dbf")};
    return {path};
}

bool read_point_fields(const std::string& path, size_t n_features, PointLayer& L, std::string& err) {
    L.fields.clear();
    L.values.assign(n_features, {});
    switch (layer_kind(path)) {
    case LayerKind::Shapefile: return read_dbf_fields(path, n_features, L, err);
    case LayerKind::GeoJSON: return read_geojson_fields(path, n_features, L, err);
    default: return read_text_fields(path, n_features, L, err);
    }
}

bool write_point_layer(const std::string& path, const PointLayer& L, std::string& err) {
    if (L.x.size() != L.y.size() || L.values.size() != L.x.size()) { err = "point layer: columns of different length"; return false; }
    for (const auto& row : L.values)
        if (row.size() != L.fields.size()) { err = "point layer: a feature without all fields"; return false; }
    switch (layer_kind(path)) {
    case LayerKind::Shapefile: return write_shapefile(path, L, err);
    case LayerKind::GeoJSON: return write_geojson(path, L, err);
    default: err = std::string("unsupported output ") + path + ": " + kLayerKindsMessage; return false;
    }
}

bool write_line_layer(const std::string& path, const LineLayer& L, std::string& err) {
    if (L.x.size() != L.y.size() || L.values.size() != L.x.size()) { err = "line layer: columns of different length"; return false; }
    for (size_t i = 0; i < L.x.size(); i++)
        if (L.values[i].size() != L.fields.size() || L.x[i].size() != L.y[i].size()) { err = "line layer: a feature without all fields, or with unpaired coordinates"; return false; }
    switch (layer_kind(path)) {
    case LayerKind::Shapefile: return write_line_shapefile(path, L, err);
    case LayerKind::GeoJSON: return write_line_geojson(path, L, err);
    default: err = std::string("unsupported output ") + path + ": " + kLineLayerKindsMessage; return false;
    }
}

bool write_polygon_layer(const std::string& path, const PolygonLayer& L, std::string& err) {
    if (L.values.size() != L.polygons.size()) { err = "polygon layer: columns of different length"; return false; }
    for (size_t i = 0; i < L.polygons.size(); i++) {
        if (L.values[i].size() != L.fields.size()) { err = "polygon layer: a feature without all fields"; return false; }
        for (const PolygonLayer::Polygon& pg : L.polygons[i])
            for (const PolygonLayer::Ring& rg : pg)
                if (rg.x.size() != rg.y.size()) { err = "polygon layer: a ring with unpaired coordinates"; return false; }
    }
    switch (layer_kind(path)) {
    case LayerKind::Shapefile: return write_polygon_shapefile(path, L, err);
    case LayerKind::GeoJSON: return write_polygon_geojson(path, L, err);
    default: err = std::string("unsupported output ") + path + ": " + kPolygonLayerKindsMessage; return false;
    }
}

bool read_line_layer(const std::string& path, LineLayer& L, std::string& err) {
    L = LineLayer();
    switch (layer_kind(path)) {
    case LayerKind::Shapefile:
        if (!read_line_shapes(path, L, err)) return false;
        L.values.assign(L.x.size(), {});
        return read_dbf_fields(path, L.x.size(), L, err);
    case LayerKind::GeoJSON: return read_line_geojson(path, L, err);
    default: err = std::string("unsupported input ") + path + ": " + kLineLayerKindsMessage; return false;
    }
}

bool read_polygon_layer(const std::string& path, PolygonLayer& L, std::string& err) {
    L = PolygonLayer();
    switch (layer_kind(path)) {
    case LayerKind::Shapefile:
        if (!read_polygon_shapes(path, L, err)) return false;
        L.values.assign(L.polygons.size(), {});
        return read_dbf_fields(path, L.polygons.size(), L, err);
    case LayerKind::GeoJSON: return read_polygon_geojson(path, L, err);
    default: err = std::string("unsupported input ") + path + ": " + kPolygonLayerKindsMessage; return false;
    }
}
}  // namespace tdx
