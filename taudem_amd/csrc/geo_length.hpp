// tiffIO::geotoLength (src/tiffIO.cpp:434-445): the lengths in metres of dlon and dlat degrees at latitude lat on the WGS84 ellipsoid, with the truncated PI the
// reference uses.  One definition for the two places that need it: the per-row cell sizes of a geographic raster (geotiff.cpp) and the segment lengths of
// the stream network layer (streamnet_net.cpp).  Host code; the transcendental functions are the host libm's.
#pragma once
#include <cmath>

namespace tdx {

// WGS84 constants and PI as src/tiffIO.h:94-96 and src/commonLib.h:76 have them
constexpr double kPI = 3.14159265359;
constexpr double kElipA = 6378137.000;
constexpr double kElipB = 6356752.314;
constexpr double kBoa = kElipB / kElipA;

inline void geo_to_length(double dlon, double dlat, double lat, double* xyc) {
    double ds2, beta, dbeta;
    dlat = dlat * kPI / 180.;
    dlon = dlon * kPI / 180.;
    lat = lat * kPI / 180.;
    beta = atan(kBoa * tan(lat));
    dbeta = dlat * kBoa * (cos(beta) / cos(lat)) * (cos(beta) / cos(lat));
    ds2 = (pow(kElipA * sin(beta), 2) + pow(kElipB * cos(beta), 2)) * pow(dbeta, 2);
    xyc[0] = kElipA * cos(beta) * std::fabs(dlon);
    xyc[1] = double(sqrt(double(ds2)));
}

}  // namespace tdx
