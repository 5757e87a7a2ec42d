// Stand-alone driver of the host files behind the stream network layer and CatchOutlets - taudem_amd/csrc/vector_layer.cpp, streamnet_net.cpp and
// catchoutlets.cpp, no library and no HIP: what tests/test_catchoutlets_host.py runs, and the program to build with -fsanitize=address,undefined when one
// of them changes.
//
//   netlayer_main roundtrip <dir>   a line layer (a line of one vertex and a null among its values included) written as <dir>/l.shp and <dir>/l.geojson and read
//                                   back: "ok" when vertices and values come back
//   netlayer_main chain <n>         a network of one outlet link and n links in a single-child chain above it, on a 1 x 1 raster: CatchOutlets' walk with
//                                   its own stack; prints the number of outlets
//   netlayer_main net               a link of one point and one of three through net_rows / net_layer: prints vertex counts and the Length field
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "catchoutlets.hpp"
#include "streamnet_net.hpp"
#include "vector_layer.hpp"

static int roundtrip(const std::string& dir) {
    tdx::LineLayer L;
    L.add_field("LINKNO", tdx::FieldType::Integer, 6);
    L.add_field("Length", tdx::FieldType::Real, 16, 1);
    L.add_field("name", tdx::FieldType::String);
    L.resize(3);
    L.x[0] = {1.5, 2.5, 4.0}; L.y[0] = {10.0, 9.0, 8.5};
    L.x[1] = {7.25}; L.y[1] = {-3.0};
    L.x[2] = {0.1, 0.2}; L.y[2] = {0.3, 0.4};
    for (size_t i = 0; i < 3; i++) { L.set(i, 0, (long long)(i + 1)); L.set(i, 2, std::string(i == 1 ? "" : "reach")); }
    L.set(0, 1, 12.5); L.set(1, 1, 0.0); L.set(2, 1, -3.5);
    for (const char* ext : {".shp", ".geojson"}) {
        std::string err;
        const std::string path = dir + "/l" + ext;
        if (!tdx::write_line_layer(path, L, err)) { printf("write: %s\n", err.c_str()); return 1; }
        tdx::LineLayer R;
        if (!tdx::read_line_layer(path, R, err)) { printf("read: %s\n", err.c_str()); return 1; }
        if (R.x != L.x || R.y != L.y || R.fields.size() != 3 || R.values.size() != 3) { printf("%s: geometry or table differs\n", ext); return 1; }
        for (size_t i = 0; i < 3; i++)
            if (strtol(R.values[i][0].c_str(), nullptr, 10) != long(i + 1) || strtod(R.values[i][1].c_str(), nullptr) != strtod(L.values[i][1].c_str(), nullptr)) {
                printf("%s: values of feature %zu differ\n", ext, i);
                return 1;
            }
    }
    std::string err;
    tdx::LineLayer R;
    if (tdx::write_line_layer(dir + "/l.kml", L, err) || tdx::read_line_layer(dir + "/l.kml", R, err)) { printf("an unknown extension was taken\n"); return 1; }
    printf("ok\n");
    return 0;
}

static int chain(long n) {
    std::vector<tdx::NetLink> links(size_t(n) + 1);
    for (long i = 0; i <= n; i++) {
        tdx::NetLink& k = links[size_t(i)];
        k.linkno = int32_t(i); k.dslinkno = int32_t(i - 1); k.uslinkno1 = i < n ? int32_t(i + 1) : -1; k.uslinkno2 = -1;
        k.doutend = double(i); k.doutstart = double(i + 1); k.uscontarea = double(n - i + 1);
        k.down_x = k.up_x = 0.5; k.down_y = k.up_y = 0.5;
    }
    tdx::FlowGrid g;
    g.nx = g.ny = 1; g.xleftedge = 0; g.ytopedge = 1; g.dlon = g.dlat = 1;
    g.p_at = [](int64_t, int64_t, int16_t& d) { d = 1; return true; };
    std::vector<tdx::CatchOutlet> out;
    std::string err;
    if (!tdx::catch_outlets(links, g, 0.5, 1, 1.5, out, err)) { printf("%s\n", err.c_str()); return 1; }
    printf("%zu %d\n", out.size(), out.empty() ? 0 : out.back().id);
    // a cycle is found, not walked for ever
    links[size_t(n)].uslinkno1 = 1;
    printf("%s\n", tdx::catch_outlets(links, g, 0.0, 1, 0.0, out, err) ? "walked a cycle" : err.c_str());
    return 0;
}

static int net() {
    const int64_t tree[18] = {0, 0, 0, -1, 1, -1, 2, -1, 2, 1, 1, 3, 0, -1, -1, 1, -1, 1};
    const double coord[20] = {5, 5, 0, 10, 900, 1, 9, 50, 14, 100, 1, 8, 40, 13, 200, 5, 5, 0, 10, 900};
    streamnet::NetRows rows;
    std::string err;
    if (!streamnet::net_rows(tree, coord, 2, 4, false, rows, err)) { printf("%s\n", err.c_str()); return 1; }
    tdx::LineLayer L;
    streamnet::net_layer(tree, 2, rows, L);
    printf("%zu %zu %s %s %zu\n", L.x[0].size(), L.x[1].size(), L.values[0][6].c_str(), L.values[1][6].c_str(), L.fields.size());
    const int64_t bad[9] = {0, 3, 4, -1, -1, -1, 1, -1, 1};
    printf("%s\n", streamnet::net_rows(bad, coord, 1, 4, false, rows, err) ? "took rows outside coord" : "refused");
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && strcmp(argv[1], "roundtrip") == 0) return roundtrip(argv[2]);
    if (argc == 3 && strcmp(argv[1], "chain") == 0) return chain(atol(argv[2]));
    if (argc == 2 && strcmp(argv[1], "net") == 0) return net();
    fprintf(stderr, "usage: netlayer_main roundtrip <dir> | chain <n> | net\n");
    return 2;
}
