// PeukerDouglas as the reference writes it (src/PeukerDouglas.cpp:109-212), on one rank: a smoothing pass into a second grid, the copy back, then the
// SEQUENTIAL scan over the 2x2 groups that clears flags in scan order.  Deliberately not the per-cell "union of the groups" form of the product's
// kernels: the two formulations check each other.  Rows -1 and ny are the partition's border rows, which hold nodata on one rank; the nodata test is
// linearpart<float>::isNodata (src/linearpart.h:471-483).
//   g++ -O2 -ffp-contract=off -shared -fPIC peuker_restate.cpp -o peuker_restate.so
#include <cmath>
#include <cstdint>
#include <vector>

namespace {

const int d1[9] = {0, 1, 1, 0, -1, -1, -1, 0, 1};
const int d2[9] = {0, 0, -1, -1, -1, 0, 1, 1, 1};
const float MINEPS = 1e-5f;

struct Grid {
    long nx, ny;
    float nodata;
    std::vector<float> v;   // rows -1 .. ny
    Grid(long nx_, long ny_, float nd) : nx(nx_), ny(ny_), nodata(nd), v(size_t(nx_) * size_t(ny_ + 2), nd) {}
    float& at(long x, long y) { return v[size_t(y + 1) * size_t(nx) + size_t(x)]; }
    bool isNodata(long x, long y) {
        if (x >= 0 && x < nx && y >= -1 && y <= ny) return std::fabs((float)(at(x, y) - nodata)) < MINEPS;
        return true;
    }
};

}  // namespace

extern "C" void pk_run(int nx, int ny, const float* fel, float nodata, const float* p, int16_t* ssout, float* smoothed) {
    Grid elev(nx, ny, nodata), selev(nx, ny, nodata);
    std::vector<int16_t> ss(size_t(nx) * size_t(ny), 0);
    for (long y = 0; y < ny; y++)
        for (long x = 0; x < nx; x++) elev.at(x, y) = fel[size_t(y) * size_t(nx) + size_t(x)];
    const int rank = 0, size = 1;
    const long elevnx = nx, elevny = ny;
    for (long y = 0; y < elevny; y++) {
        for (long x = 0; x < elevnx; x++) {
            if ((rank == 0 && y == 0) || (rank == (size - 1) && y == (elevny - 1))) {
                selev.at(x, y) = elev.at(x, y);
                ss[size_t(y) * size_t(nx) + size_t(x)] = 0;
            } else if (x == 0 || x == (elevnx - 1) || elev.isNodata(x, y)) {
                selev.at(x, y) = elev.at(x, y);
                ss[size_t(y) * size_t(nx) + size_t(x)] = 0;
            } else {
                ss[size_t(y) * size_t(nx) + size_t(x)] = 1;
                float elevwsum = p[0] * elev.at(x, y);
                float wsum = p[0];
                if (p[1] > 0.)
                    for (int k = 1; k <= 7; k = k + 2) {
                        if (!elev.isNodata(x + d1[k], y + d2[k])) {
                            elevwsum += elev.at(x + d1[k], y + d2[k]) * (p[1]);
                            wsum += p[1];
                        }
                    }
                if (p[2] > 0.)
                    for (int k = 2; k <= 8; k = k + 2) {
                        if (!elev.isNodata(x + d1[k], y + d2[k])) {
                            elevwsum += elev.at(x + d1[k], y + d2[k]) * p[2];
                            wsum += p[2];
                        }
                    }
                elevwsum = elevwsum / wsum;
                selev.at(x, y) = elevwsum;
            }
        }
    }
    for (long y = 0; y < elevny; y++)
        for (long x = 0; x < elevnx; x++) elev.at(x, y) = selev.at(x, y);
    if (smoothed)
        for (long y = 0; y < ny; y++)
            for (long x = 0; x < nx; x++) smoothed[size_t(y) * size_t(nx) + size_t(x)] = elev.at(x, y);
    auto clear = [&](long x, long y) {
        if (y >= 0 && y < ny) ss[size_t(y) * size_t(nx) + size_t(x)] = 0;   // (a border row of the flag partition: not part of the output)
    };
    for (long y = -1; y < elevny; y++) {
        for (long x = 0; x < elevnx - 1; x++) {
            float emax = elev.at(x, y);
            int iomax = 0, jomax = 0, bound = 0;
            for (int ik = 0; ik < 2; ik++)
                for (int jk = 1 - ik; jk < 2; jk++) {
                    if (elev.isNodata(x + jk, y + ik)) bound = 1;
                    else if (elev.at(x + jk, y + ik) > emax) {
                        emax = elev.at(x + jk, y + ik);
                        iomax = ik;
                        jomax = jk;
                    }
                }
            clear(x + jomax, y + iomax);
            if (bound == 1) {
                for (int ik = 0; ik < 2; ik++)
                    for (int jk = 0; jk < 2; jk++) clear(x + jk, y + ik);
            } else {
                for (int ik = 0; ik < 2; ik++)
                    for (int jk = 0; jk < 2; jk++)
                        if (elev.at(x + jk, y + ik) == emax) clear(x + jk, y + ik);
            }
        }
    }
    for (size_t i = 0; i < ss.size(); i++) ssout[i] = ss[i];
}
