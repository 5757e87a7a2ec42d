// Host side of CatchHydroGeo and InunDepth: the text files around the raster work.  Readers keep the reference's parsing (256-byte lines, strtok / atoi /
// atof, "%lf\n", "%d,%lf"), its messages on stderr and its order of checks; a reader returns false after it has printed what the reference prints
// before exit(1).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace handtables {

struct CatchList {   // src/CatchHydroGeo.cpp:128-212
    std::vector<int32_t> id;
    std::vector<double> slope, length, manning;
};
bool read_catch_list(const char* path, CatchList& out);
// src/CatchHydroGeo.cpp:230-252; false (no message: the reference crashes there) when the file cannot be opened
bool read_stages(const char* path, std::vector<double>& stage);
// derived columns + table (src/CatchHydroGeo.cpp:335-373); count / surface / bed / volume [nh][ncatch]
bool write_hydroprop(const char* path, const CatchList& cl, const std::vector<double>& stage, const std::vector<int32_t>& count, const std::vector<double>& surface,
                     const std::vector<double>& bed, const std::vector<double>& volume, const std::vector<double>& catcharea);

struct Forecast {    // src/InunDepth.cpp:111-347
    std::vector<int32_t> id;
    std::vector<double> flow;
    std::vector<float> depth;       // interpolated in double, stored as float; -9999 without two distinct bounds
    std::vector<float> catcharea;   // CatchArea_m2 of the last table row with the id, -9999 without one
};
bool read_forecast(const char* fcfile, const char* hpfile, Forecast& out);
// src/InunDepth.cpp:416-442; area[i]: inundated area at the winning row of each id (0 elsewhere)
void write_depths(const char* path, const Forecast& fc, const std::vector<float>& area);

}  // namespace handtables
