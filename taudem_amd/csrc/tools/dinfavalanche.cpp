// dinfavalanche -ang ang -fel fel -ass ass -rz rz -dfs dfs [-thresh 0.2] [-alpha 18] [-direct]   (flag surface of src/DinfAvalanchemn.cpp:48-200)
#include "cli_common.hpp"

static void usage(const char* prog) {
    printf("Simple use:\n %s <basefilename>\n", prog);
    printf("General use:\n %s -ang <angfile> -fel <felfile> -ass <assfile> -rz <rzfile> -dfs <dfsfile> [-thresh <thresh>] [-alpha <alpha>] [-direct]\n", prog);
    printf("  <angfile>  D-infinity flow direction input\n");
    printf("  <felfile>  pit-filled elevation input\n");
    printf("  <assfile>  avalanche source site input (cells > 0 are sources)\n");
    printf("  <rzfile>   runout zone output: the angle to the source, degrees\n");
    printf("  <dfsfile>  distance from the source output\n");
    printf("  -thresh <thresh>  a neighbour contributes only if its proportion is at least thresh (default 0.2)\n");
    printf("  -alpha <alpha>    the runout ends where the angle to the source falls below alpha degrees (default 18)\n");
    printf("  -direct    distance as a straight line from the source instead of along the flow path\n");
    printf("With the simple form the suffixes ang, fel, ass, rz and dfs are inserted before the extension of <basefilename>.\n");
    exit(0);
}

int main(int argc, char** argv) {
    cli::take_gpus(argc, argv);
    std::string angfile, felfile, assfile, rzfile, dfsfile, text;
    int path = 1;
    float thresh = 0.2f, alpha = 18.0f;
    if (argc < 2) { printf("Error: use either the simple form or the form with explicit file names\n"); usage(argv[0]); }
    cli::Args a(argc, argv);
    while (a.more()) {
        if (a.is("-ang")) { if (!a.value(angfile)) usage(argv[0]); }
        else if (a.is("-fel")) { if (!a.value(felfile)) usage(argv[0]); }
        else if (a.is("-ass")) { if (!a.value(assfile)) usage(argv[0]); }
        else if (a.is("-rz")) { if (!a.value(rzfile)) usage(argv[0]); }
        else if (a.is("-dfs")) { if (!a.value(dfsfile)) usage(argv[0]); }
        else if (a.is("-thresh")) { if (!a.value(text)) usage(argv[0]); sscanf(text.c_str(), "%f", &thresh); }
        else if (a.is("-alpha")) { if (!a.value(text)) usage(argv[0]); sscanf(text.c_str(), "%f", &alpha); }
        else if (a.is("-direct")) { a.flag(); path = 0; }
        else usage(argv[0]);
    }
    if (argc == 2) {
        felfile = cli::nameadd(argv[1], "fel"); angfile = cli::nameadd(argv[1], "ang"); assfile = cli::nameadd(argv[1], "ass");
        rzfile = cli::nameadd(argv[1], "rz"); dfsfile = cli::nameadd(argv[1], "dfs");
    }
    const int err = tdx_tool_dinfavalanche(angfile.c_str(), felfile.c_str(), assfile.c_str(), rzfile.c_str(), dfsfile.c_str(), thresh, alpha, path);
    return cli::finish("DinfAvalanche", err);
}
