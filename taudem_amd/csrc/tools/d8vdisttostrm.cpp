// d8vdisttostrm -p p -fel fel -src src -dist dist [-thresh N]   (flag surface of src/D8VDistToStrmmn.cpp:52-160)
#include "cli_common.hpp"

static void usage(const char* prog) {
    printf("Simple Usage:\n %s <basefilename>\n", prog);
    printf("Usage with specific file names:\n %s -p <pfile>\n", prog);
    printf("-fel <felfile> -src <srcfile> -dist <distfile> [-thresh <thresh>]\n");
    printf("<basefilename> is the name of the base digital elevation model\n");
    printf("<pfile> is the d8 flow direction input file.\n");
    printf("<felfile> is the pit filled elevation input file.\n");
    printf("<srcfile> is the stream raster input file (read as 4-byte integers: cells >= <thresh> are stream).\n");
    printf("<distfile> is the vertical distance to stream output file.\n");
    printf("The optional <thresh> is the user input threshold number (default 1).\n");
    printf("With the simple form the suffixes p, fel, src and dist are inserted before the extension of <basefilename>.\n");
    exit(0);
}

int main(int argc, char** argv) {
    cli::take_gpus(argc, argv);
    std::string pfile, felfile, srcfile, distfile;
    int thresh = 1;   // src/D8VDistToStrmmn.cpp:55
    if (argc < 2) { printf("Error: To run this program, use either the Simple Usage option or\nthe Usage with Specific file names option\n"); usage(argv[0]); }
    cli::Args a(argc, argv);
    while (a.more()) {
        if (a.is("-p")) { if (!a.value(pfile)) usage(argv[0]); }
        else if (a.is("-fel")) { if (!a.value(felfile)) usage(argv[0]); }
        else if (a.is("-src")) { if (!a.value(srcfile)) usage(argv[0]); }
        else if (a.is("-dist")) { if (!a.value(distfile)) usage(argv[0]); }
        else if (a.is("-thresh")) { if (!a.value(thresh)) usage(argv[0]); }
        else usage(argv[0]);
    }
    if (argc == 2) { pfile = cli::nameadd(argv[1], "p"); felfile = cli::nameadd(argv[1], "fel"); srcfile = cli::nameadd(argv[1], "src"); distfile = cli::nameadd(argv[1], "dist"); }
    const int err = tdx_tool_d8vdisttostrm(pfile.c_str(), felfile.c_str(), srcfile.c_str(), distfile.c_str(), thresh);
    return cli::finish("D8 vertical distance", err);
}
