// The polygon layer reader and the region table writer in a program of their own, for a build under sanitizers (tests/test_polygon_reader_main.py):
//   reader_main layer <path> [field]     "feature <i> <rings> <value of field, - without one>" and "ring x y x y ..." per ring (%.17g), or "refused: <why>"
//   reader_main table <path> <id>...     writes the region table with the script's default texts and prints its bytes
// Exit status 0 in every case: anything else is a sanitizer's report.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "region_table.hpp"
#include "vector_layer.hpp"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const std::string mode = argv[1], path = argv[2];
    std::string err;
    if (mode == "table") {
        std::vector<int32_t> ids;
        for (int k = 3; k < argc; k++) ids.push_back(int32_t(atoi(argv[k])));
        const char* texts[7] = {"2.708", "2.708", "0.0", "0.25", "30.0", "45.0", "2000.0"};
        if (!regions::write_table(path, ids.data(), int32_t(ids.size()), texts, err)) { printf("refused: %s\n", err.c_str()); return 0; }
        FILE* f = fopen(path.c_str(), "rb");
        if (!f) return 3;
        for (int c; (c = fgetc(f)) != EOF;) putchar(c);
        fclose(f);
        return 0;
    }
    tdx::PolygonLayer L;
    if (!tdx::read_polygon_layer(path, L, err)) { printf("refused: %s\n", err.c_str()); return 0; }
    std::vector<int32_t> values;
    if (argc > 3 && !regions::attribute_values(L, argv[3], values, err)) { printf("refused: %s\n", err.c_str()); return 0; }
    for (size_t i = 0; i < L.polygons.size(); i++) {
        size_t nr = 0;
        for (const auto& pg : L.polygons[i]) nr += pg.size();
        if (argc > 3) printf("feature %zu %zu %d\n", i, nr, values[i]);
        else printf("feature %zu %zu -\n", i, nr);
        for (const auto& pg : L.polygons[i])
            for (const auto& rg : pg) {
                printf("ring");
                for (size_t k = 0; k < rg.x.size(); k++) printf(" %.17g %.17g", rg.x[k], rg.y[k]);
                printf("\n");
            }
    }
    return 0;
}
