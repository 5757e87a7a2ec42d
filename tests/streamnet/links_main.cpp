/* The product's host link builder (taudem_amd/csrc/streamnet_links.cpp) as a stand-alone program: reads the compact stream-cell arrays that
 * the restatement dumps (sn_dump_compact), builds the links and writes the -tree and -coord files.  Built by tests/test_streamnet_links.py; built
 * by hand with -fsanitize=address,undefined it is the sanitizer check of the link builder (no GPU, nothing loaded into an interpreter):
 *     links_main <compact.bin> <nx> <dxA> <dyA> <left> <cell width> <top> <cell height> <tree.txt> <coord.txt> */
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "streamnet_links.hpp"

template <class T>
static bool read_n(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc != 11) { fprintf(stderr, "usage: links_main compact.bin nx dxA dyA left width top height tree.txt coord.txt\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    int64_t n = 0;
    if (!f || fread(&n, 8, 1, f) != 1 || n < 0) { fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
    std::vector<int64_t> idx;
    std::vector<int16_t> p;
    std::vector<float> fel, ad8, len;
    std::vector<int32_t> outlet, recv;
    std::vector<uint8_t> flags;
    const size_t m = size_t(n);
    if (!read_n(f, idx, m) || !read_n(f, p, m) || !read_n(f, fel, m) || !read_n(f, ad8, m) || !read_n(f, len, m) || !read_n(f, outlet, m) || !read_n(f, recv, m) ||
        !read_n(f, flags, m)) {
        fprintf(stderr, "%s is short\n", argv[1]);
        return 1;
    }
    fclose(f);
    streamnet::Compact C;
    C.n = n; C.idx = idx.data(); C.p = p.data(); C.fel = fel.data(); C.ad8 = ad8.data(); C.len = len.data(); C.outlet = outlet.data(); C.recv = recv.data();
    C.flags = flags.data();
    const double gt[4] = {atof(argv[5]), atof(argv[6]), atof(argv[7]), atof(argv[8])};
    streamnet::Links L;
    streamnet::build_links(C, atoll(argv[2]), atof(argv[3]), atof(argv[4]), gt, L);
    FILE* ft = fopen(argv[9], "w");
    FILE* fc = fopen(argv[10], "w");
    if (!ft || !fc) { fprintf(stderr, "cannot write the outputs\n"); return 1; }
    for (size_t i = 0; i + 9 <= L.tree.size(); i += 9) {
        for (int k = 0; k < 9; k++) fprintf(ft, "\t%lld", (long long)L.tree[i + size_t(k)]);
        fputc('\n', ft);
    }
    for (size_t i = 0; i + 5 <= L.coord.size(); i += 5)
        fprintf(fc, "\t%f\t%f\t%f\t%f\t%f\n", L.coord[i], L.coord[i + 1], L.coord[i + 2], L.coord[i + 3], L.coord[i + 4]);
    fclose(ft);
    fclose(fc);
    return 0;
}
