// moveoutletstostrm -p p -src src -o outlets -om movedoutlets [-md maxdist] [-lyrname n] [-lyrno i] [-omlyr n]
// (flag surface of src/MoveOutletsToStrmmn.cpp:65-190; there is no simple form).  The layer options are accepted and ignored.
#include "cli_common.hpp"

static void usage(const char* prog) {
    printf("Incorrect input.\n");
    printf("Use with specific file names:\n %s -p <pfile>\n", prog);
    printf("-src <srcfile> -o <outletsshapefile> -om <outletsmoved>\n");
    printf("[-md <max dist>]\n");
    printf("<pfile> is the name of the D8 flow direction file (input).\n");
    printf("<srcfile> is the name of the stream raster file (input).\n");
    printf("<outletsshapefile> is the name of the outlet shape file (input).\n");
    printf("<outletsmoved> is the name of the moved outlet shape file (output).\n");
    printf("<max dist> is the maximum number of grid cells to move an outlet (input).\n");
    printf("Default <max dist> is 50 if not input.\n");
    exit(0);
}

int main(int argc, char** argv) {
    cli::take_gpus(argc, argv);
    std::string pfile, srcfile, outlets, outletslayer, moved, movedlayer;
    int maxdist = 50, uselyrname = 0, lyrno = 0;
    if (argc < 9) {
        printf("No simple use case for this function.\n");
        usage(argv[0]);
    }
    cli::Args a(argc, argv);
    while (a.more()) {
        if (a.is("-p")) { if (!a.value(pfile)) usage(argv[0]); }
        else if (a.is("-src")) { if (!a.value(srcfile)) usage(argv[0]); }
        else if (a.is("-o")) { if (!a.value(outlets)) usage(argv[0]); }
        else if (a.is("-lyrno")) { if (!a.value(lyrno)) usage(argv[0]); }
        else if (a.is("-lyrname")) { if (!a.value(outletslayer)) usage(argv[0]); uselyrname = 1; }
        else if (a.is("-om")) { if (!a.value(moved)) usage(argv[0]); }
        else if (a.is("-omlyr")) { if (!a.value(movedlayer)) usage(argv[0]); }
        else if (a.is("-md")) { if (!a.value(maxdist)) usage(argv[0]); }
        else usage(argv[0]);
    }
    const int err = tdx_tool_moveoutletstostrm(pfile.c_str(), srcfile.c_str(), outlets.c_str(), outletslayer.c_str(), uselyrname, lyrno, moved.c_str(), movedlayer.c_str(), maxdist);
    if (err == 4 || err == 1) { fflush(stdout); return err; }   // MPI_Abort(MCW, 4): p does not match src; exit(1): the outlet source cannot be opened
    if (err == TDX_ERR_ARG) return 2;                           // an output this build cannot write: said on stderr, nothing was read
    return cli::finish("Move outlets to stream", err);
}
