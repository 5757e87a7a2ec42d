// catchoutlets -p p (-net streamnet | -tree tree -coord coord) -o outlets [-mindist d] [-gwstartno n] [-minarea a]
// (flag surface and defaults of src/CatchOutletsmn.cpp:57-188 - mindist 0, minarea 0, gwstartno 1, no simple form - plus -tree / -coord, this project's
// streamnet outputs, in place of -net).  Host code: no GPU is touched, --gpus is accepted and means nothing.
#include "cli_common.hpp"

static void usage(const char* prog) {
    printf("Incorrect input.\n");
    printf("Use with specific file names:\n %s -p <pfile>\n", prog);
    printf("-net <streamnet source> [-netlyr <stream net layer>] -o <outletsshapefile>\n");
    printf("[-lyrno <layer number for outlet> -lyrname <layer name for outlet> -mindist <Min distance between outlets>]\n");
    printf("<pfile> is the name of the D8 flow direction file (input).\n");
    printf("<stream net source> is the name of the stream network shapefile data source (input).\n");
    printf("<stream net layer> is the name of the stream network shapefile data layer (optional input).\n");
    printf("<outletsshapefile> is the name of the outlet shape file (input).\n");
    printf("<layer number> is the layer number for the outlets layer in the shapefile as a data source (output).\n");
    printf("<layer name> is the layer name for the outlets layer in the shapefile as a data source (output).\n");
    printf("<mindist> is the minimum distance between outlets (input).\n");
    printf("Default <mindist> is 0 if not input.\n");
    printf("In place of -net: -tree <treefile> -coord <coordfile>, the text files streamnet writes.  [-gwstartno <first Id>] [-minarea <min contributing area>]\n");
    exit(0);
}

int main(int argc, char** argv) {
    cli::take_gpus(argc, argv);
    std::string pfile, net, tree, coord, outlets;
    double mindist = 0.0, minarea = 0.0;
    int gwstartno = 1;
    if (argc < 7) {
        printf("To few input arguments.\n");
        usage(argv[0]);
    }
    int i = 1;
    while (argc > i) {
        std::string* s = strcmp(argv[i], "-p") == 0 ? &pfile : strcmp(argv[i], "-net") == 0 ? &net : strcmp(argv[i], "-tree") == 0 ? &tree : strcmp(argv[i], "-coord") == 0 ? &coord
                         : strcmp(argv[i], "-o") == 0 ? &outlets : nullptr;
        double* d = strcmp(argv[i], "-mindist") == 0 ? &mindist : strcmp(argv[i], "-minarea") == 0 ? &minarea : nullptr;
        const bool g = strcmp(argv[i], "-gwstartno") == 0;
        if (!s && !d && !g) usage(argv[0]);
        i++;
        if (argc <= i) usage(argv[0]);
        if (s) *s = argv[i];
        else if (d) sscanf(argv[i], "%lf", d);
        else sscanf(argv[i], "%d", &gwstartno);
        i++;
    }
    if (net.empty() == (tree.empty() && coord.empty()) || tree.empty() != coord.empty()) {
        fprintf(stderr, "catchoutlets: give the stream network either as -net <line layer> or as -tree <file> -coord <file>\n");
        usage(argv[0]);
    }
    const int err = tdx_tool_catchoutlets(pfile.c_str(), net.c_str(), tree.c_str(), coord.c_str(), outlets.c_str(), mindist, gwstartno, minarea);
    if (err == TDX_ERR_ARG) return 2;   // an extension no reader or writer exists for, a layer without a needed field: said on stderr
    return cli::finish("Catchment Outlets", err);
}
