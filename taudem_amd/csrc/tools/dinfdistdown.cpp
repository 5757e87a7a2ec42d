// dinfdistdown -ang ang -fel fel -slp slp -src src [-wg wg] -dd dd [-m ave v] [-nc]   (flag surface of src/DinfDistDownmn.cpp:44-213)
#include "cli_common.hpp"

static void usage(const char* prog) {
    printf("Simple use:\n %s <basefilename>\n", prog);
    printf("General use:\n %s -ang <angfile> -fel <felfile> -slp <slpfile> -src <srcfile> [-wg <wgfile>] -dd <ddfile> [-m <stat> <type>] [-nc]\n", prog);
    printf("  <angfile>  D-infinity flow direction input\n");
    printf("  <felfile>  pit-filled elevation input (not read for type h)\n");
    printf("  <slpfile>  D-infinity slope input (accepted, not read)\n");
    printf("  <srcfile>  stream raster input (cells >= 1 are stream)\n");
    printf("  <wgfile>   optional weight input: multiplies the horizontal step to each receiver (types h, p, s)\n");
    printf("  <ddfile>   distance down to the stream output\n");
    printf("  -m <stat> <type>  statistic ave | max | min and distance type h | v | p | s, in either order (default: ave h)\n");
    printf("  -nc        no edge contamination check\n");
    printf("With the simple form the suffixes ang, fel, slp, src, wg and dd are inserted before the extension of <basefilename>.\n");
    exit(0);
}

// one token of -m: a distance type or a statistic (src/DinfDistDownmn.cpp:133-196: anything else is ignored)
static void method_token(const char* t, int& statmethod, int& typemethod) {
    if (strcmp(t, "h") == 0) typemethod = 0;
    else if (strcmp(t, "v") == 0) typemethod = 1;
    else if (strcmp(t, "p") == 0) typemethod = 2;
    else if (strcmp(t, "s") == 0) typemethod = 3;
    if (strcmp(t, "ave") == 0) statmethod = 0;
    else if (strcmp(t, "max") == 0) statmethod = 1;
    else if (strcmp(t, "min") == 0) statmethod = 2;
}

int main(int argc, char** argv) {
    cli::take_gpus(argc, argv);
    std::string angfile, felfile, slpfile, srcfile, wfile, ddfile;
    int statmethod = 0, typemethod = 0, usew = 0, concheck = 1;
    if (argc < 2) { printf("Error: use either the simple form or the form with explicit file names\n"); usage(argv[0]); }
    cli::Args a(argc, argv);
    while (a.more()) {
        if (a.is("-ang")) { if (!a.value(angfile)) usage(argv[0]); }
        else if (a.is("-fel")) { if (!a.value(felfile)) usage(argv[0]); }
        else if (a.is("-slp")) { if (!a.value(slpfile)) usage(argv[0]); }
        else if (a.is("-src")) { if (!a.value(srcfile)) usage(argv[0]); }
        else if (a.is("-wg")) { if (!a.value(wfile)) usage(argv[0]); usew = 1; }
        else if (a.is("-dd")) { if (!a.value(ddfile)) usage(argv[0]); }
        else if (a.is("-m")) {
            if (a.i + 2 >= argc) usage(argv[0]);
            method_token(argv[a.i + 1], statmethod, typemethod);
            method_token(argv[a.i + 2], statmethod, typemethod);
            a.i += 3;
        } else if (a.is("-nc")) { a.flag(); concheck = 0; }
        else usage(argv[0]);
    }
    if (argc == 2) {   // (the simple form never uses the weight file: usew stays 0)
        angfile = cli::nameadd(argv[1], "ang"); felfile = cli::nameadd(argv[1], "fel"); slpfile = cli::nameadd(argv[1], "slp");
        srcfile = cli::nameadd(argv[1], "src"); wfile = cli::nameadd(argv[1], "wg"); ddfile = cli::nameadd(argv[1], "dd");
    }
    const int err = tdx_tool_dinfdistdown(angfile.c_str(), felfile.c_str(), slpfile.c_str(), wfile.c_str(), srcfile.c_str(), ddfile.c_str(), statmethod, typemethod,
                                          usew, concheck);
    return cli::finish("area", err);   // (the reference's message: "area error %d")
}
