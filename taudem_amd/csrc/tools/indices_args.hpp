// The argument surfaces of twi, slopearea, slopearearatio, lengtharea and setregion (src/TWImn.cpp, src/SlopeAreamn.cpp, src/SlopeAreaRatiomn.cpp,
// src/LengthAreamn.cpp, src/SetRegionmn.cpp) as one table-driven parser without a library call in it, so that tests/indices/args_main.cpp can run it
// alone:  one word after the program name = "simple use", the three file names come from nameadd(); more words = "-flag value" pairs in any order,
// "-par a b" for the two tools that take parameters, "-id n" for setregion, which has no simple use.  Anything else is a usage error.
#pragma once
#include <cstdint>

#include "cli_common.hpp"

namespace cli {

struct IndexTool {
    const char* flag[3];     // input, input, output - in the order of the tool function's arguments
    const char* suffix[3];   // simple use; nullptr: the tool has none
    bool has_par;
    float par[2];            // the defaults of -par
    bool has_id;
};

// twigrid(slopefile, areafile, twifile); slopearea(slopefile, scafile, safile, p); atanbgrid(slopefile, areafile, atanbfile);
// lengtharea(plenfile, ad8file, ssfile, p); setregion(fdrfile, regiongwfile, newfile, regionID)
static const IndexTool kTwi = {{"-slp", "-sca", "-twi"}, {"slp", "sca", "twi"}, false, {0.0f, 0.0f}, false};
static const IndexTool kSlopeArea = {{"-slp", "-sca", "-sa"}, {"slp", "sca", "sa"}, true, {2.0f, 1.0f}, false};
static const IndexTool kSlopeAreaRatio = {{"-slp", "-sca", "-sar"}, {"slp", "sca", "sar"}, false, {0.0f, 0.0f}, false};
static const IndexTool kLengthArea = {{"-plen", "-ad8", "-ss"}, {"plen", "ad8", "ss"}, true, {0.03f, 1.3f}, false};
static const IndexTool kSetRegion = {{"-p", "-gw", "-out"}, {nullptr, nullptr, nullptr}, false, {0.0f, 0.0f}, true};

struct IndexArgs {
    std::string file[3];
    float par[2] = {0.0f, 0.0f};
    int32_t id = 1;
};

// false: print the usage
inline bool parse_index_args(const IndexTool& t, int argc, char** argv, IndexArgs& a) {
    a.par[0] = t.par[0];
    a.par[1] = t.par[1];
    a.id = 1;
    if (argc < 2) return false;
    if (argc == 2) {
        if (!t.suffix[0]) return false;
        for (int k = 0; k < 3; k++) a.file[k] = nameadd(argv[1], t.suffix[k]);
        return true;
    }
    int i = 1;
    while (argc > i) {
        int k = 0;
        while (k < 3 && strcmp(argv[i], t.flag[k]) != 0) k++;
        if (k < 3) {
            i++;
            if (argc <= i) return false;
            a.file[k] = argv[i++];
        } else if (t.has_par && strcmp(argv[i], "-par") == 0) {
            i++;
            if (argc <= i + 1) return false;
            sscanf(argv[i++], "%f", &a.par[0]);   // a word that is no number leaves the value as it was, as in the reference
            sscanf(argv[i++], "%f", &a.par[1]);
        } else if (t.has_id && strcmp(argv[i], "-id") == 0) {
            i++;
            if (argc <= i) return false;
            int v = a.id;
            sscanf(argv[i++], "%d", &v);
            a.id = int32_t(v);
        } else return false;
    }
    return true;
}

inline int index_usage(const IndexTool& t, const char* prog) {
    if (t.suffix[0]) printf("Simple use:\n %s <basefilename>   (the suffixes '%s', '%s' and '%s' are added to it)\n", prog, t.suffix[0], t.suffix[1], t.suffix[2]);
    printf("Use with specific file names:\n %s %s <input file> %s <input file> %s <output file>", prog, t.flag[0], t.flag[1], t.flag[2]);
    if (t.has_par) printf(" [-par <a> <b>]   (default %g %g)", t.par[0], t.par[1]);
    if (t.has_id) printf(" [-id <region identifier>]   (default 1)");
    printf(" [--gpus <n>]\n");
    return 0;
}

}  // namespace cli
