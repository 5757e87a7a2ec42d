// dinfdistup -ang ang -fel fel -slp slp [-wg wg] -du du [-m ave h] [-nc] [-thresh t]   (flag surface of src/DinfDistUpmn.cpp:51-220)
#include "cli_common.hpp"

static void usage(const char* prog) {
    printf("Simple use:\n %s <basefilename>\n", prog);
    printf("General use:\n %s -ang <angfile> -fel <felfile> -slp <slpfile> [-wg <wgfile>] -du <dufile> [-m <stat> <type>] [-nc] [-thresh <t>]\n", prog);
    printf("  <angfile>  D-infinity flow direction input\n");
    printf("  <felfile>  pit-filled elevation input (not read for type h)\n");
    printf("  <slpfile>  D-infinity slope input (accepted, not read)\n");
    printf("  <wgfile>   optional weight input: multiplies the horizontal step from each contributor (types h, p, s)\n");
    printf("  <dufile>   distance up to the ridge output\n");
    printf("  -m <stat> <type>  statistic ave | max | min and distance type h | v | p | s, in either order (default: ave h)\n");
    printf("  -nc        no edge contamination check\n");
    printf("  -thresh <t>  a neighbour contributes only if its proportion exceeds t (default 0)\n");
    printf("With the simple form the suffixes ang, fel, slp, wg and du are inserted before the extension of <basefilename>.\n");
    exit(0);
}

// one token of -m: a distance type or a statistic (src/DinfDistUpmn.cpp:125-186: anything else is ignored)
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
    std::string angfile, felfile, slpfile, wfile, dufile, thresh_text;
    int statmethod = 0, typemethod = 0, usew = 0, concheck = 1;
    float thresh = 0.0f;
    if (argc < 2) { printf("Error: use either the simple form or the form with explicit file names\n"); usage(argv[0]); }
    cli::Args a(argc, argv);
    while (a.more()) {
        if (a.is("-ang")) { if (!a.value(angfile)) usage(argv[0]); }
        else if (a.is("-fel")) { if (!a.value(felfile)) usage(argv[0]); }
        else if (a.is("-slp")) { if (!a.value(slpfile)) usage(argv[0]); }
        else if (a.is("-wg")) { if (!a.value(wfile)) usage(argv[0]); usew = 1; }
        else if (a.is("-du")) { if (!a.value(dufile)) usage(argv[0]); }
        else if (a.is("-m")) {
            if (a.i + 2 >= argc) usage(argv[0]);
            method_token(argv[a.i + 1], statmethod, typemethod);
            method_token(argv[a.i + 2], statmethod, typemethod);
            a.i += 3;
        } else if (a.is("-nc")) { a.flag(); concheck = 0; }
        else if (a.is("-thresh")) { if (!a.value(thresh_text)) usage(argv[0]); sscanf(thresh_text.c_str(), "%f", &thresh); }
        else usage(argv[0]);
    }
    if (argc == 2) {   // (the simple form never uses the weight file: usew stays 0)
        angfile = cli::nameadd(argv[1], "ang"); felfile = cli::nameadd(argv[1], "fel"); slpfile = cli::nameadd(argv[1], "slp");
        wfile = cli::nameadd(argv[1], "wg"); dufile = cli::nameadd(argv[1], "du");
    }
    const int err = tdx_tool_dinfdistup(angfile.c_str(), felfile.c_str(), slpfile.c_str(), wfile.c_str(), dufile.c_str(), statmethod, typemethod, usew, concheck,
                                        thresh);
    return cli::finish("area", err);   // (the reference's message: "area error %d")
}
