// A stand-alone program over the point-layer code (taudem_amd/csrc/vector_layer.cpp and outlets.cpp), for tests/test_vector_layer.py and for runs
// under -fsanitize=address,undefined (host code with a main of its own: nothing is loaded into an interpreter).
//   vector_main <directory>          writes a.shp (+ .shx, .dbf) and b.geojson there, reads both back with the outlet reader and the field reader,
//                                    writes each once more from what was read and compares the bytes; prints "ok"
//   vector_main carry <in> <out>     what moveoutletstostrm does around its walk: the points and ALL fields of <in>, Dist_moved = i - 1 appended, to <out>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "outlets.hpp"
#include "vector_layer.hpp"

static std::string slurp(const std::string& p) {
    std::ifstream f(p, std::ios::binary);
    std::stringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

static int fail(const std::string& what) {
    fprintf(stderr, "vector_main: %s\n", what.c_str());
    return 1;
}

static bool read_back(const std::string& path, tdx::PointLayer& L, std::string& err) {
    std::vector<int> id;
    if (!tdx::read_outlets(path, L.x, L.y, id, err)) return false;
    return tdx::read_point_fields(path, L.x.size(), L, err);
}

int main(int argc, char** argv) {
    std::string err;
    if (argc == 4 && strcmp(argv[1], "carry") == 0) {
        tdx::PointLayer L;
        if (!read_back(argv[2], L, err)) return fail(err);
        const size_t k = L.add_field("Dist_moved", tdx::FieldType::Integer, 6);
        for (size_t i = 0; i < L.x.size(); i++) L.set(i, k, (long long)i - 1);
        if (!tdx::write_point_layer(argv[3], L, err)) return fail(err);
        return 0;
    }
    if (argc != 2) return fail("usage: vector_main <directory> | vector_main carry <in> <out>");
    const std::string dir = argv[1];
    tdx::PointLayer L;
    const size_t ki = L.add_field("id", tdx::FieldType::Integer), kr = L.add_field("ad8", tdx::FieldType::Real), ks = L.add_field("name", tdx::FieldType::String),
                 kd = L.add_field("Dist_moved", tdx::FieldType::Integer, 6);
    L.resize(300);
    for (size_t i = 0; i < 300; i++) {
        L.x[i] = 1000.0 + 0.1 * double(i); L.y[i] = 5000.0 - double(i) / 3.0;
        L.set(i, ki, (long long)(i * 7919) - 1000000);
        L.set(i, kr, double(i) * 1.25 - 17.0);
        L.set(i, ks, std::string(i % 90, char('a' + i % 26)) + (i % 5 == 0 ? "\"\\\n" : ""));
        L.set(i, kd, (long long)(i % 52) - 1);
    }
    if (tdx::layer_kind(dir + "/x.kml") != tdx::LayerKind::None || tdx::write_point_layer(dir + "/x.kml", L, err)) return fail("an unsupported extension was taken");
    for (const char* name : {"/a.shp", "/b.geojson"}) {
        const std::string path = dir + name, again = dir + "/again" + std::string(name).substr(2);
        if (!tdx::write_point_layer(path, L, err)) return fail(err);
        tdx::PointLayer R;
        if (!read_back(path, R, err)) return fail(err);
        if (R.x != L.x || R.y != L.y || R.fields.size() != L.fields.size()) return fail(path + ": points or fields differ after reading back");
        for (size_t k = 0; k < L.fields.size(); k++)
            if (R.fields[k].name != L.fields[k].name || R.fields[k].type != L.fields[k].type) return fail(path + ": field " + L.fields[k].name + " changed");
        if (!tdx::write_point_layer(again, R, err)) return fail(err);
        for (const std::string& f : tdx::layer_files(path)) {
            const std::string g = dir + "/again" + f.substr(dir.size() + 2);
            if (slurp(f) != slurp(g)) return fail(f + ": written again from what was read, the bytes differ");
            remove(g.c_str());
        }
    }
    // a truncated .dbf and a broken GeoJSON are errors, not crashes
    { std::ofstream t(dir + "/t.shp", std::ios::binary); t << slurp(dir + "/a.shp"); }
    { std::ofstream t(dir + "/t.dbf", std::ios::binary); t << slurp(dir + "/a.dbf").substr(0, 1000); }
    tdx::PointLayer T;
    if (read_back(dir + "/t.shp", T, err)) return fail("a truncated .dbf was accepted");
    { std::ofstream t(dir + "/t.geojson"); t << slurp(dir + "/b.geojson").substr(0, 777); }
    tdx::PointLayer U;
    if (read_back(dir + "/t.geojson", U, err)) return fail("a broken GeoJSON was accepted");
    for (const char* n : {"/t.shp", "/t.dbf", "/t.geojson"}) remove((dir + n).c_str());
    printf("ok\n");
    return 0;
}
