// The region parameter table of the SINMAP parameter region grid (include/taudem_amd_regions.h): what sinmapsi reads as -calpar.  Plain C++, no device.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "vector_layer.hpp"

namespace regions {
extern const char* const kTableHeader;   // "SiID,tmin,tmax,cmin,cmax,phimin,phimax,SoilDens"
// The header line, then "id,t0,...,t6" per id in the order given; the seven texts are written as they are.  false + err: the file cannot be written.
bool write_table(const std::string& path, const int32_t* ids, int32_t n_ids, const char* const* seven_texts, std::string& err);
// The region ids of a polygon layer: the integer values of `field`, one per feature, each in 1 .. 32767.  false + err (naming the feature): no such
// field, the field name FID (a shapefile's record number is no attribute), a null, a value that is no integer, a value outside the range.
bool attribute_values(const tdx::PolygonLayer& layer, const std::string& field, std::vector<int32_t>& values, std::string& err);
}  // namespace regions
